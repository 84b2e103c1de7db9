"""Row-wise multi-label NMS (dyk_nms_rows) on the CPU: symbols, struct layout against the C compiler, the workspace formula of
include/dyk_hip.h and its bound, argument checks (none of these calls reaches a launch: every descriptor here is invalid in
exactly one way), the default capacity of the wrapper, and the candidate counts the GPU tests rely on.  No GPU."""
import ctypes
import inspect
import os
import subprocess

import pytest

import nms_rows_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def _p2(c):
    p = 1
    while p < c:
        p <<= 1
    return p


def _up(x, m=256):
    return (x + m - 1) // m * m


def test_symbols_and_signatures():
    from dyk import lib
    h = lib.load()
    assert hasattr(h, "dyk_nms_rows") and hasattr(h, "dyk_nms_rows_workspace_bytes")
    assert len(lib.SIGNATURES["dyk_nms_rows_workspace_bytes"][1]) == 2        # (N, cand_cap): no class count to depend on
    assert lib.DykNmsRowsDesc._fields_[:len(lib.DykNmsDesc._fields_)] == lib.DykNmsDesc._fields_
    assert [f[0] for f in lib.DykNmsRowsDesc._fields_[-2:]] == ["cand_cap", "n_cand"]
    hdr = open(os.path.join(ROOT, "include", "dyk_hip.h")).read()
    assert "int64_t dyk_nms_rows_workspace_bytes(int32_t N, int32_t cand_cap);" in hdr
    assert "int dyk_nms_rows(const DykNmsRowsDesc* desc, int32_t flags, void* stream);" in hdr
    assert h.dyk_abi_version() == 5                                          # nothing that existed changed


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from dyk import lib
    names = ["DykNmsRowsDesc", "DykNmsDesc"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dyk_hip.h"', "int main(void){"]
    for s in names:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
    for f, _ in lib.DykNmsRowsDesc._fields_:
        lines.append('printf("DykNmsRowsDesc.%s %%zu\\n", offsetof(DykNmsRowsDesc, %s));' % (f, f))
    for f, _ in lib.DykNmsDesc._fields_:
        lines.append('printf("DykNmsDesc.%s %%zu\\n", offsetof(DykNmsDesc, %s));' % (f, f))
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for s in names:
        cls = getattr(lib, s)
        assert int(out[s]) == ctypes.sizeof(cls), s
        for f, _ in cls._fields_:
            assert int(out["%s.%s" % (s, f)]) == getattr(cls, f).offset, (s, f)
    for f, _ in lib.DykNmsDesc._fields_:                                     # the shared fields sit at the same offsets
        assert out["DykNmsRowsDesc.%s" % f] == out["DykNmsDesc.%s" % f], f


@pytest.mark.parametrize("N,cap", [(1, 1), (1, 8192), (63, 100), (700, 27143), (1500, 8192), (3000, 8192), (20160, 20160),
                                   (20160, 8192), (20161, 65537), (1 << 20, 1 << 20)])
def test_workspace_formula_and_bound(N, cap):
    """header: roundup(8 * P(cand_cap) + 28 * cand_cap, 256) + roundup(8 * N, 256); issue: at most the keys and candidates of a
    best-class call over cand_cap rows plus 16 bytes per row, rounded up to 256"""
    from dyk import lib
    h = lib.load()
    got = int(h.dyk_nms_rows_workspace_bytes(N, cap))
    single = int(h.dyk_nms_workspace_bytes(cap, 6, 0))
    assert single == _up(8 * _p2(cap) + 28 * cap)
    assert got == single + _up(8 * N)
    assert got <= _up(single + 16 * N)
    assert got % 256 == 0


def test_workspace_of_the_readme_batch_is_a_fiftieth_of_the_per_pair_one():
    from dyk import lib
    h = lib.load()
    rows = int(h.dyk_nms_rows_workspace_bytes(20160, 20160))
    pairs = int(h.dyk_nms_workspace_bytes(20160, 85, 1))
    print("N = 20160: row-wise %d bytes per image, per-pair at 80 classes %d bytes (x %.1f)" % (rows, pairs, pairs / rows))
    assert rows < pairs / 50
    assert 16 * pairs > 950e6 and 16 * rows < 18e6                           # the 991 MB and the 13 to 16 MB of the README batch


def _almost_valid(lib, keep):
    """a descriptor whose every check passes; the caller breaks exactly one thing before the call (the pointers are host
    memory: a call that passed every check would launch on them, so no test calls it unbroken)"""
    h = lib.load()
    d = lib.DykNmsRowsDesc()
    buf = ctypes.create_string_buffer(64)
    keep.append(buf)
    a = ctypes.addressof(buf)
    d.pred, d.out, d.out_rows, d.counts, d.ws, d.n_cand = a, a, a, a, a, a
    d.B, d.N, d.no, d.conf_thres, d.iou_thres = 2, 1500, 85, 0.5, 0.6
    d.multi_label, d.agnostic, d.max_num, d.n_classes = 1, 0, 100, 0
    d.cand_cap = 8192
    d.ws_per_image = int(h.dyk_nms_rows_workspace_bytes(1500, 8192))
    return d


BREAK = {
    "cand_cap_0": lambda d: setattr(d, "cand_cap", 0),
    "cand_cap_negative": lambda d: setattr(d, "cand_cap", -5),
    "ws_one_byte_short": lambda d: setattr(d, "ws_per_image", d.ws_per_image - 1),
    "ws_sized_for_a_smaller_capacity": lambda d: setattr(d, "cand_cap", 8193),
    "n_cand_null": lambda d: setattr(d, "n_cand", None),
    "pred_null": lambda d: setattr(d, "pred", None),
    "counts_null": lambda d: setattr(d, "counts", None),
    "ws_null": lambda d: setattr(d, "ws", None),
    "B_0": lambda d: setattr(d, "B", 0),
    "N_0": lambda d: setattr(d, "N", 0),
    "no_5": lambda d: setattr(d, "no", 5),
    "max_num_513": lambda d: setattr(d, "max_num", 513),
    "n_classes_17": lambda d: setattr(d, "n_classes", 17),
    "conf_thres_negative": lambda d: setattr(d, "conf_thres", -0.1),
    "conf_thres_nan": lambda d: setattr(d, "conf_thres", float("nan")),
    "best_class_call": lambda d: setattr(d, "multi_label", 0),
    "one_class": lambda d: setattr(d, "no", 6),
}


@pytest.mark.parametrize("what", sorted(BREAK))
def test_bad_descriptors_are_rejected_without_a_gpu(what):
    from dyk import lib
    h = lib.load()
    keep = []
    for flags in (0, lib.NMS_MERGE):
        d = _almost_valid(lib, keep)
        BREAK[what](d)
        assert h.dyk_nms_rows(ctypes.byref(d), flags, None) == ERR_ARG, (what, flags)


def test_null_descriptor_and_unknown_flags():
    from dyk import lib
    h = lib.load()
    assert h.dyk_nms_rows(None, 0, None) == ERR_ARG
    assert h.dyk_nms_rows(None, lib.NMS_MERGE, None) == ERR_ARG
    keep = []
    for flags in (2, 4, lib.NMS_MERGE | 2, -2, 1 << 30):
        d = _almost_valid(lib, keep)                                         # valid but for the flags: refused before anything
        assert h.dyk_nms_rows(ctypes.byref(d), flags, None) == ERR_ARG, flags


def test_default_capacity_of_the_wrapper():
    from build_utils import utils
    from dyk import detect
    assert detect.nms_default_candidates(20160) == 20160                      # what a best-class call holds
    assert detect.nms_default_candidates(8193) == 8193
    assert detect.nms_default_candidates(8192) == 8192
    assert detect.nms_default_candidates(700) == 8192                         # the floor
    assert detect.nms_default_candidates(1) == 8192
    for fn in (detect.non_max_suppression, utils.non_max_suppression):
        assert inspect.signature(fn).parameters["candidates"].default is None
    assert set(detect.nms_route_counts()) == {"image", "rows", "rows_overflow"}
    c = detect.nms_route_counts()
    c["rows"] += 1                                                           # a copy: not a switch
    assert detect.nms_route_counts()["rows"] == c["rows"] - 1
    assert isinstance(detect.NMS_ROWS_MIN_NC, int) and detect.NMS_ROWS_MIN_NC >= 2


def test_candidate_counts_of_the_matrix():
    """the relations the GPU tests rely on, recomputed from the inputs"""
    from dyk import detect
    n = {}
    for name, c in RC.MATRIX.items():
        alive, cand = RC.candidate_counts(RC.pred(name), c["conf"])
        print("%-8s N %5d nc %3d conf %.2f: alive rows / candidates %s" % (name, c["N"], c["nc"], c["conf"],
                                                                          "  ".join("%d/%d" % ac for ac in zip(alive, cand))))
        assert min(alive) > 0 and all(k > a for a, k in zip(alive, cand))     # rows give several candidates: multi-label
        n[name] = cand
    for name in ("s80", "s80_cap", "s33", "s20", "ties3"):                   # fit the default capacity
        assert max(n[name]) <= detect.nms_default_candidates(RC.MATRIX[name]["N"]), name
    assert min(n["s365"]) > detect.nms_default_candidates(700)               # every image overflows it
    assert n["s80_cap"][0] <= 2100 < min(n["s80_cap"][1:])                   # capacity 2100: image 0 fits, 1 and 2 do not
    _, filt = RC.candidate_counts(RC.pred("s80"), RC.MATRIX["s80"]["conf"], RC.S80_CLASSES)
    assert all(0 < f < k for f, k in zip(filt, n["s80"])) and len(RC.S80_CLASSES) == 16
