"""The ctypes layouts of the structures of dyk_resize_pad_pairs (dyk/lib.py) against what the C compiler makes of
include/dyk_hip.h: sizeof and the offset of EVERY field, through a tiny gcc-built probe.  No compute, no GPU.
(tests/test_abi.py keeps its fixed list of the older structures.)"""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = ["DykResizePadRec", "DykResizePadDesc"]


def test_struct_layouts_match_the_c_compiler(tmp_path):
    from dyk import lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dyk_hip.h"', "int main(void){"]
    for s in STRUCTS:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for name, _ in getattr(lib, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, name, s, name))
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
    assert ctypes.sizeof(lib.DykResizePadRec) == 48             # what the wrapper sends up per image


def test_the_entry_is_declared_bound_and_exported():
    from dyk import lib
    assert "dyk_resize_pad_pairs" in lib.SIGNATURES
    assert hasattr(lib.load(), "dyk_resize_pad_pairs")
    assert "dyk_resize_pad_pairs" in open(os.path.join(ROOT, "include", "dyk_hip.h")).read()
