"""Generates tests/golden/optim_step_bits.json: sha256 digests of what the fused optimizer steps leave in memory, taken from
the library named by DYK_LIB (default: the in-tree build) on an MI355X.  tests/test_gpu_optim_step_bits.py holds the library
under test to every digest.  The committed file was written by the commit BEFORE the six step kernels of csrc/optim.hip /
csrc/optim_guard.hip became one template and the four step() bodies of dyk/optim.py became one; regenerate it only when the
bits of a step are meant to change.

Section `abi`: one launch of dyk_adam_step / dyk_sgd_step, their _guarded and their _groups forms on the buffers of
tests/test_gpu_optim.py (guard bands included in the digests of p, m, v, wc, g), inputs of oracle.optim.input_family:
  plain    n = 4, 3200 without and with a binary mask that has frozen runs, BIG (ragged second grid-stride sweep) with the mask;
           step 1 (SGD's first-step rule) and 1000, zero_grad 0 / 1, the bf16 copy on / off
  guarded  n = 3200 and BIG, grad_scale 1/65536, records with coef 0.75 at applied = 1 and 1000, and with skip = 1 at zero_grad 0 / 1
  groups   the layouts `one`, `interleaved`, `big` of tests/test_gpu_optim_groups.py, without and with a record, a mask byte
           above the group count
Section `objects`: three step() calls of the optimizer classes on the smallest model of the model tests, the flat gradient buffer
filled from a seeded generator before each (no forward or backward pass): P and the moment buffers after the last one.
Every entry also carries a digest of its inputs: a test that fails there says that the inputs changed, not the kernel.

    DYK_LIB=/path/to/libdyk_hip.so python tests/golden/make_optim_step_bits.py [--out FILE]
"""
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "double-yolo-kaist_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "optim_step_bits.json")
OUTPUTS = ("p", "m", "v", "wc", "g")
SEED = 44                                      # (the BIG inputs of this seed at grad_scale 1/8 are shared with test_gpu_optim_groups.py)
BETAS = (0.937, 0.999)
_DIGESTS = {}


def sha(*parts):
    h = hashlib.sha256()
    for x in parts:
        h.update(x.encode() if isinstance(x, str) else x)
    return h.hexdigest()


def _tensor_sha(t):
    import torch
    return sha(t.detach().reshape(-1).contiguous().view(torch.uint8).cpu().numpy())


# ---------------------------------------------------------------------------------------------- section `abi`
def abi_cases():
    """-> {id: dict}; the id is the dict's items joined"""
    out = []
    small = list(itertools.product((1, 1000), (0, 1), (False, True)))
    for kind in ("adam", "sgd"):
        for shape in ("4", "3200", "3200_masked", "big_masked"):
            for step, zero_grad, wc in (small if shape != "big_masked" else [(1, 0, False), (1000, 1, True)]):
                out.append(dict(entry="plain", kind=kind, shape=shape, step=step, zero_grad=zero_grad, wc=wc))
        records = [dict(applied=1, skip=0, zero_grad=1), dict(applied=1000, skip=0, zero_grad=0),
                   dict(applied=3, skip=1, zero_grad=0), dict(applied=3, skip=1, zero_grad=1)]
        for shape in ("3200", "3200_masked"):
            out += [dict(entry="guarded", kind=kind, shape=shape, wc=True, **r) for r in records]
        out += [dict(entry="guarded", kind=kind, shape="big_masked", wc=True, **r) for r in (records[1], records[3])]
        for layout in ("one", "interleaved"):
            for rec, step in itertools.product((False, True), (1, 1000)):
                out.append(dict(entry="groups", kind=kind, layout=layout, rec=rec, step=step, skip=0, zero_grad=int(step == 1), wc=step == 1))
        out.append(dict(entry="groups", kind=kind, layout="interleaved", rec=True, step=3, skip=1, zero_grad=1, wc=True))
        out.append(dict(entry="groups", kind=kind, layout="interleaved", rec=False, step=3, skip=0, zero_grad=1, wc=True, count=2))
        out.append(dict(entry="groups", kind=kind, layout="big", rec=False, step=2, skip=0, zero_grad=1, wc=True))
        out.append(dict(entry="groups", kind=kind, layout="big", rec=True, step=1000, skip=0, zero_grad=1, wc=True))
    return {"-".join("%s=%s" % kv for kv in c.items()): c for c in out}


def _inputs(kind, n, beta1, grad_scale):
    """input_family through the per-process cache of test_gpu_optim_groups.py, and the digests of its arrays"""
    import test_gpu_optim_groups as G
    key = (kind, n, SEED, grad_scale)
    before = G.inputs(kind, n, SEED, beta1, grad_scale)
    if key not in _DIGESTS:
        _DIGESTS[key] = "".join(sha(before[k]) for k in ("p", "g", "m", "v"))
    return before, _DIGESTS[key]


def run_abi_case(c):
    """one launch -> (digest of the inputs, {buffer: digest of the whole buffer after the launch})"""
    import numpy as np
    import test_gpu_optim as T
    import test_gpu_optim_groups as G
    from dyk import lib as L
    kind, entry = c["kind"], c["entry"]
    table = rec = None
    if entry == "groups":
        n, mask, groups = G.layout(c["layout"], kind)
        groups = groups[:c.get("count", len(groups))]
        gs = 1 / 8
        h = G.hyper(kind, c["step"], gs)
        table = G.table_of(groups)
        if c["rec"]:
            rec = G.record(h, c["step"], 0.75, c["skip"])
    else:
        n = {"4": 4, "3200": 3200, "big": T.BIG}[c["shape"].split("_")[0]]
        mask = T._frozen_mask(n) if c["shape"].endswith("_masked") else None
        gs = 1 / 8 if entry == "plain" else 1 / 65536
        h = T._h(**dict(T.ADAM if kind == "adam" else T.SGD, grad_scale=gs, step=c.get("step", 0)))
        if entry == "guarded":
            rec = G.record(h, c["applied"], 0.75, c["skip"])
    before, digest = _inputs(kind, n, h["beta1"], 1 / 8 if n == T.BIG else gs)
    b = T.Bufs(n, **(dict(before) if mask is None else dict(before, mask=mask)))
    if entry == "groups":
        d = G.desc(b, dict(h, step=0 if c["rec"] else c["step"]), zero_grad=c["zero_grad"], wc=c["wc"])
    else:
        d = b.desc(h, mask=mask is not None, zero_grad=c["zero_grad"], wc=c["wc"])
    digest = sha(digest, b"" if mask is None else np.ascontiguousarray(mask), bytes(d)[L.DykOptimDesc.n.offset:],
                 b"" if table is None else bytes(table), b"" if rec is None else rec.cpu().numpy(), repr(sorted(c.items())))
    if entry == "groups":
        rc = G.launch(kind, d, table, rec)
    else:
        rc = G.launch_existing(kind, d, rec)
    assert rc == 0, (c, rc)
    return digest, {k: _tensor_sha(b.full[k]) for k in OUTPUTS}


# ---------------------------------------------------------------------------------------------- section `objects`
OBJECT_MODES = ("adam", "sgd", "adam_frozen", "adam_guarded", "sgd_groups_lr_rewritten", "adamw_groups_guarded",
                "adam_guarded_state_dict", "clip_grad_norm_frozen")
FROZEN_LAYERS = 10
_MODEL = {}


def _model(frozen):
    """the smallest cfg of tests/test_gpu_optim_groups_model.py, built once per process; every mode starts from the same P, with
    the first FROZEN_LAYERS layers frozen or not, G attached and zero"""
    import torch
    from helpers import C1
    from test_gpu_harness import _model as make
    if not _MODEL:
        m = make(C1)                                       # (torch.manual_seed(0) inside)
        with torch.no_grad():
            m.engine.store.adopt(torch.device("cuda", 0))
        _MODEL.update(m=m, P0=m.engine.store.P.clone(), P0_sha=_tensor_sha(m.engine.store.P), blocks={})
    m = _MODEL["m"]
    head = {id(p) for idx in range(FROZEN_LAYERS) for p in m.module_list[idx].parameters()}
    for p in m.parameters():
        p.requires_grad_(not (frozen and id(p) in head))
    st = m.engine.store
    with torch.no_grad():
        st.P.copy_(_MODEL["P0"])
    for e in st.entries:
        e.param.grad = None
    st.attach_grads()
    return m


BLOCK = (1 << 20) + 4 * 257                    # elements of the seeded block that tiles G: no multiple of an entry's 64-element alignment


def _fill(st, t, plant_inf=False):
    """the flat gradient buffer of step t (1-based): a block of seeded normals, a decade smaller every step, repeated over the
    buffer (drawn once per process and step); plant_inf: +Inf in the last trainable element -> digest of what was written"""
    import numpy as np
    import torch
    if t not in _MODEL["blocks"]:
        block = (np.random.default_rng(7 + t).standard_normal(BLOCK) * 10.0 ** (-1 - t)).astype(np.float32)
        _MODEL["blocks"][t] = (torch.from_numpy(block).cuda(), sha(block))
    block, digest = _MODEL["blocks"][t]
    with torch.no_grad():
        st.G.copy_(block.repeat(-(-st.total // BLOCK))[:st.total])
        if plant_inf:
            live = next(e for e in reversed(st.entries) if e.param.requires_grad)
            st.G[live.offset + live.numel - 1] = float("inf")
    return "%s x %d inf %s" % (digest, st.total, plant_inf)


def run_object_mode(mode):
    """-> (digest of the inputs, {name: digest}, grad_stats of the last step or None)"""
    import torch
    from dyk import optim as O
    m = _model(frozen="frozen" in mode)
    st = m.engine.store
    ins, out, stats = [mode, _MODEL["P0_sha"]], {}, None
    if mode == "clip_grad_norm_frozen":
        ins.append(_fill(st, 1))
        norm = O.clip_grad_norm_(m, 1e-3)
        out = dict(G=_tensor_sha(st.G), norm=_tensor_sha(norm))
        return sha(*ins), out, stats
    groups = lambda wd, bias_lr: O.yolo_param_groups(m, wd, bias_lr=bias_lr)
    guard = dict(max_grad_norm=1e-3, skip_nonfinite=True)   # (the norms are about 1e-2 * sqrt(total) and less: every step is clipped)
    make = {
        "adam": lambda: O.FusedAdam(m, lr=1e-3, betas=BETAS, weight_decay=5e-4),
        "sgd": lambda: O.FusedSGD(m, lr=1e-2, momentum=0.937, weight_decay=5e-4),
        "adam_frozen": lambda: O.FusedAdam(m, lr=1e-3, betas=BETAS, weight_decay=5e-4),
        "adam_guarded": lambda: O.FusedAdam(m, lr=1e-3, betas=BETAS, weight_decay=5e-4, **guard),
        "sgd_groups_lr_rewritten": lambda: O.FusedSGD(m, lr=1e-2, momentum=0.937, param_groups=groups(5e-4, 2e-2)),
        "adamw_groups_guarded": lambda: O.FusedAdamW(m, lr=1e-3, betas=BETAS, param_groups=groups(1e-2, 2e-3), **guard),
        "adam_guarded_state_dict": lambda: O.FusedAdam(m, lr=1e-3, betas=BETAS, weight_decay=5e-4, **guard),
    }[mode]
    opt = make()

    def step(o, t, plant_inf=False):
        ins.append(_fill(st, t, plant_inf))
        o.step()

    def digests(o, name):
        out.update({"%s.P" % name: _tensor_sha(st.P), "%s.m" % name: _tensor_sha(o._m)})
        if o._v is not None:
            out["%s.v" % name] = _tensor_sha(o._v)
    for t in (1, 2, 3):
        if mode == "sgd_groups_lr_rewritten" and t > 1:
            for k, g in enumerate(opt.param_groups):
                g["lr"] = g["lr"] * (0.5 + 0.25 * k)
        step(opt, t, plant_inf=(mode == "adam_guarded" and t == 2))
    digests(opt, "step3")
    if mode == "adam_guarded_state_dict":
        sd = opt.state_dict()
        fresh = make()
        fresh.load_state_dict(sd)                           # (a record is allocated at its first step, from the loaded count)
        step(fresh, 4)
        digests(fresh, "fresh4")
        opt.load_state_dict(sd)                             # (its record exists: the count is written into it)
        step(opt, 5)
        digests(opt, "again5")
        opt = fresh
    if "guarded" in mode:
        s = opt.grad_stats(wait=True)
        stats = dict(applied_steps=s["applied_steps"], skipped_steps=s["skipped_steps"])
    torch.cuda.synchronize()
    return sha(*ins), out, stats


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library, so that both use the HIP runtime torch brings)
    from dyk import lib as L
    lib = L.load()
    abi = {}
    for cid, c in abi_cases().items():
        abi[cid] = dict(zip(("in", "out"), run_abi_case(c)))
    objects = {}
    for mode in OBJECT_MODES:
        objects[mode] = dict(zip(("in", "out", "stats"), run_object_mode(mode)))
    with open(a.out, "w") as f:
        f.write('{"library": "%s",\n "abi": {\n' % lib.dyk_build_sha().decode())
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in abi.items()))
        f.write('\n },\n "objects": {\n')
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in objects.items()))
        f.write("\n }}\n")
    print("%s: %d launches, %d optimizer modes, library %s" % (a.out, len(abi), len(objects), lib.dyk_build_sha().decode()))


if __name__ == "__main__":
    main()
