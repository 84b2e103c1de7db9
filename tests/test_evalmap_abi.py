"""Layout of DykEvalMatchDesc: the ctypes structure of dyk/lib.py against the C compiler's view of include/dyk_hip.h, every
field (sizeof / offsetof through a tiny gcc-built probe, as tests/test_abi.py does for the other descriptors).  No GPU."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from dyk import lib as L
    cls = L.DykEvalMatchDesc
    names = [f[0] for f in cls._fields_]
    src = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dyk_hip.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(DykEvalMatchDesc));']
    lines += ['printf("%s %%zu\\n", offsetof(DykEvalMatchDesc, %s));' % (n, n) for n in names]
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    for n in names:
        assert int(out[n]) == getattr(cls, n).offset, n
    assert L.EVAL_MAX_THR == 16 and L.EVAL_MAX_GT == 1024 and L.load().dyk_abi_version() == 5
