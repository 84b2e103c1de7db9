"""The ctypes layouts of the descriptors of dyk_anchor_assign, dyk_anchor_median and dyk_anchor_fitness (dyk/lib.py) against
what the C compiler makes of include/dyk_hip.h: sizeof and the offset of EVERY field, through a tiny gcc-built probe; the
constants; the entries declared, bound and exported.  No compute, no GPU."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = ["DykAnchorAssignDesc", "DykAnchorMedianDesc", "DykAnchorFitnessDesc"]
ENTRIES = ["dyk_anchor_assign", "dyk_anchor_median_ws_bytes", "dyk_anchor_median", "dyk_anchor_fitness_ws_bytes", "dyk_anchor_fitness"]
CONSTS = {"DYK_ANCHOR_MAX_K": "ANCHOR_MAX_K", "DYK_ANCHOR_MAX_N": "ANCHOR_MAX_N", "DYK_ANCHOR_MAX_G": "ANCHOR_MAX_G",
          "DYK_ANCHOR_FIT_ITEM": "ANCHOR_FIT_ITEM"}


def test_struct_layouts_and_constants_match_the_c_compiler(tmp_path):
    from dyk import lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dyk_hip.h"', "int main(void){"]
    for s in STRUCTS:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for name, _ in getattr(lib, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, name, s, name))
    for c in CONSTS:
        lines.append('printf("%s %%ld\\n", (long)(%s));' % (c, c))
    lines.append("return 0;}")
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for s in STRUCTS:
        cls = getattr(lib, s)
        assert int(out[s]) == ctypes.sizeof(cls), "sizeof(%s): C %s vs ctypes %d" % (s, out[s], ctypes.sizeof(cls))
        for name, _ in cls._fields_:
            assert int(out["%s.%s" % (s, name)]) == getattr(cls, name).offset, "%s.%s" % (s, name)
    for c, py in CONSTS.items():
        assert int(out[c]) == getattr(lib, py), c
    assert lib.ANCHOR_MAX_N == 2 ** 27 - 1


def test_the_entries_are_declared_bound_and_exported():
    from dyk import lib
    header = open(os.path.join(ROOT, "include", "dyk_hip.h")).read()
    h = lib.load()
    for e in ENTRIES:
        assert e in lib.SIGNATURES and hasattr(h, e) and (" %s(" % e) in header, e


def test_workspace_size_and_refusals_need_no_device():
    """NULL or out-of-range arguments return DYK_ERR_ARG (-1) before anything touches a device"""
    from dyk import lib
    h = lib.load()
    assert h.dyk_anchor_fitness_ws_bytes(1, 1, 1) == 24                      # one slot: 8 + 8 K + 4, rounded up to 8
    assert h.dyk_anchor_fitness_ws_bytes(1025, 7, 9) == 7 * 2 * (8 + 72 + 4)
    for bad in ((0, 1, 1), (2 ** 27, 1, 1), (1, 0, 1), (1, 4097, 1), (1, 1, 0), (1, 1, 33)):
        assert h.dyk_anchor_fitness_ws_bytes(*bad) == 0, bad
    assert h.dyk_anchor_assign(None, None) == -1 and h.dyk_anchor_median(None, None) == -1 and h.dyk_anchor_fitness(None, None) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(wh=p, c=p, nearest=p, stats=p, N=1, K=1, elem_bytes=4)
    for change in (dict(wh=None), dict(c=None), dict(nearest=None), dict(stats=None), dict(N=0), dict(N=2 ** 27), dict(K=0), dict(K=33),
                   dict(elem_bytes=2), dict(wh=p + 4, elem_bytes=8), dict(nearest=p + 2)):
        assert h.dyk_anchor_assign(ctypes.byref(lib.DykAnchorAssignDesc(**dict(ok, **change))), None) == -1, change
    assert h.dyk_anchor_median_ws_bytes(9) == 18 * (32 + 1024) and h.dyk_anchor_median_ws_bytes(0) == 0 and h.dyk_anchor_median_ws_bytes(33) == 0
    ok = dict(wh=p, c=p, nearest=p, ws=p, ws_bytes=2 * (32 + 1024), N=1, K=1, elem_bytes=8)
    for change in (dict(wh=None), dict(c=None), dict(nearest=None), dict(ws=None), dict(ws_bytes=2111), dict(ws=p + 4), dict(N=0), dict(K=33),
                   dict(elem_bytes=0), dict(c=p + 4)):
        assert h.dyk_anchor_median(ctypes.byref(lib.DykAnchorMedianDesc(**dict(ok, **change))), None) == -1, change
    ok = dict(wh=p, a=p, ws=p, fit_boxes=p, fit_anchors=p, hit_boxes=p, hit_anchors=p, ws_bytes=24, thr=0.25, N=1, K=1, G=1, elem_bytes=4)
    for change in (dict(wh=None), dict(a=None), dict(ws=None), dict(fit_boxes=None), dict(fit_anchors=None), dict(hit_boxes=None),
                   dict(hit_anchors=None), dict(ws_bytes=16), dict(thr=float("nan")), dict(thr=float("inf")), dict(N=0), dict(K=33), dict(G=0),
                   dict(G=4097), dict(elem_bytes=3), dict(a=p + 4), dict(ws=p + 4)):
        assert h.dyk_anchor_fitness(ctypes.byref(lib.DykAnchorFitnessDesc(**dict(ok, **change))), None) == -1, change
