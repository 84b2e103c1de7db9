"""Generates tests/golden/dwconv_bits.json: sha256 digests of what the depthwise kernels of csrc/dwconv.hip leave in memory, taken
from the library named by DYK_LIB (default: the in-tree build) on an MI355X.  tests/test_gpu_dwconv_bits.py holds the library
under test to every digest.  The committed file was written by the commit BEFORE the file got one tile geometry, one route per
entry point and lost its dead code; regenerate it only when the bits of a kernel are meant to change.

The cases and inputs are those of tests/dwconv_cases.py, the buffers those of tests/test_gpu_dwconv_elements.py (sentinel-filled,
guard rows and padding channels inside every digest):
  f       the forward of matrix("f") in every dtype, launched with the case's statistics slots as the element suite does: y
  d       the data gradient of matrix("d"), plain and accumulate: dx
  w       the weight-gradient PLANES of matrix("w"), and of the three cases at a plane base offset by one float
  pre     normalise + activation on load, six activations x k 3, 5: the forward, the tiled weight-gradient planes (stride 1) and
          the row-kernel weight-gradient planes (stride 2)
  res     the data gradient with the fused BatchNorm-backward reduce on the inputs of tests/test_gpu_conv.py's test: da only
  single  four single-workgroup launches in which every address receives exactly ONE atomic onto zero, so that the bits are
          fixed: statistics of the tiled and of the generic forward, atomic dw of the tiled and of the row weight gradient
Buffers that several workgroups add onto with atomics -- the BatchNorm statistics and the non-plane dw of every other case --
have no fixed summation order; they stay out of this file and under the fp64 bounds of the element suite.
Every entry also carries a digest of its inputs: a test that fails there says that the inputs changed, not the kernel.

    DYK_LIB=/path/to/libdyk_hip.so python tests/golden/make_dwconv_bits.py [--out FILE]
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "double-yolo-kaist_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "dwconv_bits.json")
UNALIGNED = ["c72_k3p1_1x17", "c24_k5p2_23x17", "c264_k3p1s2_9x12"]
RES_CASES = [(2, 72, 17, 23, 3), (1, 120, 12, 20, 5), (2, 16, 40, 36, 3)]
RES_ACTS = ["hard-swish", "relu", "linear"]


def sha(*parts):
    h = hashlib.sha256()
    for x in parts:
        h.update(x.encode() if isinstance(x, str) else x)
    return h.hexdigest()


def _t(t):
    """bytes of a tensor, on either device"""
    import torch
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def _E():
    import test_gpu_dwconv_elements as E
    return E


def _problem_sha(p):
    return sha(repr(tuple(p.case)), str(p.dtype), *[_t(t) for t in (p.x, p.w, p.dy, p.old) if t is not None])


# ---------------------------------------------------------------------------------------------- the launches
def run_forward(p, slots, keep_stats=False):
    E = _E()
    c = p.case
    Ho, Wo = E.out_hw(c)
    xb = E._in_buf(c, p.dtype, p.x)
    yb = E.Buf(c.B, Ho, Wo, c.C, p.dtype)
    wd = p.w.cuda()
    d = E._desc(xb.t, yb.t, wd, c)
    st = None
    if slots:
        st = E._stats_buf(slots, c.C)
        d.stats, d.stats_slots = st[1:].data_ptr(), slots
    E._sync_ok(E._lib().dyk_dwconv_fwd(ctypes.byref(d), None), "dyk_dwconv_fwd")
    out = dict(y=sha(_t(yb.flat)))
    if keep_stats:
        out["stats"] = sha(_t(st))
    return out


def run_dgrad(p, accumulate):
    E = _E()
    c = p.case
    gb = E._in_buf(c, p.dtype, p.dy)
    ob = E.Buf(c.B, c.H, c.W, c.C, p.dtype)
    if accumulate:
        ob.put(p.old)
    wd = p.w.cuda()
    d = E._desc(ob.t, gb.t, wd, c)
    d.flags = 1 if accumulate else 0
    E._sync_ok(E._lib().dyk_dwconv_dgrad(ctypes.byref(d), None), "dyk_dwconv_dgrad")
    return dict(dx=sha(_t(ob.flat)))


def run_wgrad(p, part_shift=0, atomic=False):
    """planes: the plane buffer between its guards (atomic: dw itself, for the single-workgroup cases)"""
    import torch
    E = _E()
    c = p.case
    kk = c.k * c.k
    xb = E._in_buf(c, p.dtype, p.x)
    gb = E._in_buf(c, p.dtype, p.dy, second=True)
    dwb = E.Buf(1, 1, kk, c.C, torch.float32, ld=c.C)
    dwb.t.zero_()
    d = E._desc(xb.t, gb.t, None, c)
    d.dw = dwb.t.data_ptr()
    if atomic:
        E._sync_ok(E._lib().dyk_dwconv_wgrad(ctypes.byref(d), None), "dyk_dwconv_wgrad")
        return dict(dw=sha(_t(dwb.flat)))
    rows = E._lib().dyk_dwconv_wgrad_rows(ctypes.byref(d))
    assert rows >= 1
    n = rows * kk * c.C
    flat = torch.full((64 + n + 64,), E.SENTINEL, dtype=torch.float32, device="cuda")
    part = flat[64 + part_shift:64 + part_shift + n]
    part.fill_(float("nan"))
    d.part = part.data_ptr()
    E._sync_ok(E._lib().dyk_dwconv_wgrad(ctypes.byref(d), None), "dyk_dwconv_wgrad(planes)")
    return dict(rows=rows, planes=sha(_t(flat)), dw=sha(_t(dwb.flat)))


def run_pre(act, k):
    """-> (digest of the inputs, {forward, tiled planes (stride 1), row planes (stride 2)}) with DykDwDesc.pre on the raw tensor"""
    import torch
    E = _E()
    ins, out = ["pre", act, str(k)], {}
    for stride in (1, 2):
        c, ub, zb, gb, w, pre, code = E._pre_setup(act, k, stride)
        ins += [_t(ub.flat), _t(gb.flat), _t(w), _t(pre), str(code)]
        Ho, Wo = E.out_hw(c)
        if stride == 1:
            yb = E.Buf(c.B, Ho, Wo, c.C, torch.bfloat16)
            d = E._desc(ub.t, yb.t, w, c)
            d.pre, d.pre_act = pre.data_ptr(), code
            E._sync_ok(E._lib().dyk_dwconv_fwd(ctypes.byref(d), None), "dyk_dwconv_fwd(pre)")
            out["y"] = sha(_t(yb.flat))
        d = E._desc(ub.t, gb.t, None, c)
        dw = torch.zeros(k * k, c.C, device="cuda")
        d.dw = dw.data_ptr()
        d.pre, d.pre_act = pre.data_ptr(), code
        rows = E._lib().dyk_dwconv_wgrad_rows(ctypes.byref(d))
        part = torch.full((rows + 2, k * k, c.C), E.SENTINEL, device="cuda")
        part[1:1 + rows] = float("nan")
        d.part = part[1:].data_ptr()
        E._sync_ok(E._lib().dyk_dwconv_wgrad(ctypes.byref(d), None), "dyk_dwconv_wgrad(pre)")
        out["planes_s%d" % stride] = sha(str(rows), _t(part))
    return sha(*ins), out


def run_res(case, act):
    """the inputs of test_depthwise_dgrad_with_fused_batchnorm_backward_reduce (tests/test_gpu_conv.py) -> da (the sums are
    atomics of several workgroups)"""
    import torch
    from dyk import ops
    E = _E()
    B, C, H, W, k = case
    pad = k // 2
    g = torch.Generator().manual_seed(21)
    w = torch.randn(C, 1, k, k, generator=g) / k
    dy = torch.randn(B, C, H, W, generator=g).bfloat16().float()
    u = (torch.randn(B, C, H, W, generator=g) * 2).bfloat16().float()
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    mean, rstd = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    cpad = (C + 31) // 32 * 32
    dyd = ops.to_nhwc(dy.cuda(), torch.bfloat16, cpad=cpad)
    ud = ops.to_nhwc(u.cuda(), torch.bfloat16, cpad=cpad)
    wt = w.reshape(C, k * k).t().contiguous().cuda()
    ob = E.Buf(B, H, W, C, torch.bfloat16, ld=cpad)
    slots = 4
    red = torch.zeros(slots, 2, C, dtype=torch.float64, device="cuda")
    bn = torch.cat([scale, shift, mean, rstd]).cuda().contiguous()
    d = ops._dw_desc(ob.t, dyd, wt, k, 1, pad, C)
    d.res, d.ldr, d.bn, d.act = ud.data_ptr(), cpad, bn.data_ptr(), ops.ACT_CODES[act]
    d.stats, d.stats_slots = red.data_ptr(), slots
    E._sync_ok(E._lib().dyk_dwconv_dgrad(ctypes.byref(d), None), "dyk_dwconv_dgrad(res)")
    return sha("res", repr(case), act, _t(dyd), _t(ud), _t(wt), _t(bn)), dict(da=sha(_t(ob.flat)))


# ---------------------------------------------------------------------------------------------- single-workgroup cases
def single_cases():
    from dwconv_cases import Case
    return {
        "stats_tiled": (Case("single_stats_tiled", 1, 24, 5, 9, 3, 1, 1, 1, "f", False), "bf16"),
        "stats_generic": (Case("single_stats_generic", 1, 24, 1, 9, 3, 2, 1, 1, "f", False), "bf16"),
        "dw_tiled": (Case("single_dw_tiled", 1, 24, 5, 9, 3, 1, 1, 0, "w", False), "bf16"),
        "dw_row": (Case("single_dw_row", 1, 8, 1, 9, 7, 1, 3, 0, "w", False), "bf16"),
    }


def single_problem(name):
    """inputs as dwconv_cases.problem draws them (no reference: these cases are held to recorded bits only)"""
    import torch
    from dwconv_cases import DTYPES, Problem, out_hw
    from oracle import dwconv as O
    c, dt = single_cases()[name]
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(2000 + sorted(single_cases()).index(name))
    Ho, Wo = out_hw(c)
    x = O.store(torch.randn(c.B, c.C, c.H, c.W, generator=g), dtype).float()
    w = (torch.randn(c.k * c.k, c.C, generator=g) / c.k).contiguous()
    dy = O.store(torch.randn(c.B, c.C, Ho, Wo, generator=g), dtype).float()
    return Problem(c, dtype, x, w, dy, None, None)


def assert_single_workgroup(name):
    """the premise of the fixed bits, from the geometry: one tile and one channel group (tiled kernels), one workgroup row (generic
    and row kernels; the row kernel's grid.z = kernel rows write disjoint taps)"""
    E = _E()
    c, dt = single_cases()[name]
    if E._tiled(c, dt):
        tiles, groups, planes = E._wgrad_geometry(c)
        assert (tiles, groups, planes) == (1, 1, 1), (name, tiles, groups, planes)
    elif "w" in c.ops:
        assert E._wgrad_row_planes(c, dt) == 1 and c.C // 8 <= 32, name
    else:
        assert c.B * E.out_hw(c)[0] == 1 and c.C // 8 <= 32, name
    assert c.slots in (0, 1)


def run_single(name):
    assert_single_workgroup(name)
    p = single_problem(name)
    if name.startswith("stats"):
        out = run_forward(p, 1, keep_stats=True)
    else:
        out = run_wgrad(p, atomic=True)
    return _problem_sha(p), out


# ---------------------------------------------------------------------------------------------- the table of cases
def cases():
    """-> {id: (section, arguments)}"""
    from dwconv_cases import ACTS, matrix
    out = {}
    for cid, dt in matrix("f"):
        out["f-%s-%s" % (cid, dt)] = ("f", (cid, dt))
    for cid, dt in matrix("d"):
        for acc in (False, True):
            out["d-%s-%s-%s" % (cid, dt, "accumulate" if acc else "plain")] = ("d", (cid, dt, acc))
    for cid, dt in matrix("w"):
        out["w-%s-%s" % (cid, dt)] = ("w", (cid, dt, 0))
    for cid in UNALIGNED:
        out["w-%s-bf16-unaligned" % cid] = ("w", (cid, "bf16", 1))
    for act in ACTS:
        for k in (3, 5):
            out["pre-%s-k%d" % (act, k)] = ("pre", (act, k))
    for case in RES_CASES:
        for act in RES_ACTS:
            out["res-%s-%s" % ("x".join(map(str, case)), act)] = ("res", (case, act))
    for name in single_cases():
        out["single-%s" % name] = ("single", (name,))
    return out


def run_case(section, args):
    """-> (digest of the inputs, {buffer: digest})"""
    from dwconv_cases import problem
    if section == "f":
        p = problem(*args)
        return _problem_sha(p), run_forward(p, 0 if args[1] == "f16" else p.case.slots)
    if section == "d":
        p = problem(args[0], args[1])
        return _problem_sha(p), run_dgrad(p, args[2])
    if section == "w":
        p = problem(args[0], args[1])
        return _problem_sha(p), run_wgrad(p, part_shift=args[2])
    if section == "pre":
        return run_pre(*args)
    if section == "res":
        return run_res(*args)
    return run_single(*args)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library, so that both use the HIP runtime torch brings)
    from dyk import lib as L
    lib = L.load()
    table = {}
    for cid, (section, args) in cases().items():
        table[cid] = dict(zip(("in", "out"), run_case(section, args)))
    with open(a.out, "w") as f:
        f.write('{"library": "%s",\n "cases": {\n' % lib.dyk_build_sha().decode())
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table.items()))
        f.write("\n }}\n")
    print("%s: %d cases, library %s" % (a.out, len(table), lib.dyk_build_sha().decode()))


if __name__ == "__main__":
    main()
