"""Writes tests/golden/anchor_cluster.npz: what the reference's other_utils/anchor_cluster.py computes for fixed seeded inputs.
Runs only where the reference tree is present (REF below, read-only); the tests read the .npz and never the reference.
`lxml`, which the reference imports for its VOC reader and which is not installed, is stubbed in sys.modules; nothing of the
reference's text is copied -- its functions are imported and called.

Per N in (257, 4099), k = 9: boxes = exp(RandomState(0).randn(N, 2) * 0.6 + 3.3) as float32; np.random.seed(1); the final
centres of its k_means; its anchor_fitness on the fp64-promoted boxes and centres at thr = 0.25 in both argument orders
(as defined: boxes first; as its anchor_cluster calls it: anchors first).  The generator asserts that numpy raised no warning
and that no cluster was empty in any iteration (tests/anchor_ref.py replays the same initial centres and reports empties)."""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_import import REF  # noqa: E402  (where the reference checkout lies; DYK_REFERENCE_ROOT overrides it)

REF = os.environ.get("DYK_REFERENCE_ROOT", REF)
THR, K, SIZES = 0.25, 9, (257, 4099)


def import_reference():
    lx = types.ModuleType("lxml")
    lx.etree = types.ModuleType("lxml.etree")
    sys.modules.setdefault("lxml", lx)
    sys.modules.setdefault("lxml.etree", lx.etree)
    for name in list(sys.modules):
        if name == "other_utils" or name.startswith("other_utils."):
            del sys.modules[name]
    sys.path = [p for p in sys.path if not p.rstrip("/").endswith("double-yolo-kaist_amd")]
    sys.path.insert(0, REF)
    import other_utils.anchor_cluster as ref
    assert os.path.abspath(ref.__file__).startswith(REF)
    return ref


def main():
    ref = import_reference()
    sys.path.insert(0, os.path.dirname(HERE))
    import anchor_ref
    out = {"thr": np.float64(THR), "k": np.int32(K), "sizes": np.array(SIZES, np.int32)}
    for n in SIZES:
        wh = np.exp(np.random.RandomState(0).randn(n, 2) * 0.6 + 3.3).astype(np.float32)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            np.random.seed(1)
            c = ref.k_means(wh, K)
        assert c.dtype == np.float32 and np.isfinite(c).all()
        np.random.seed(1)
        init = wh[np.random.choice(n, K, replace=False)]
        _, iters, empties = anchor_ref.k_means(wh, init=init)
        assert not empties, "a cluster emptied for N = %d: %r" % (n, empties)
        wh64, c64 = wh.astype(np.float64), c.astype(np.float64)
        f_def, r_def = ref.anchor_fitness(wh64, c64, THR)        # as defined: (whs, anchors, thr)
        f_swp, r_swp = ref.anchor_fitness(c64, wh64, THR)        # as anchor_cluster calls it
        out["centres_%d" % n] = c
        out["iterations_%d" % n] = np.int32(iters)
        out["fit_boxes_%d" % n] = np.float64(f_def)
        out["hit_boxes_%d" % n] = np.int32(round(float(r_def) * n))
        out["fit_anchors_%d" % n] = np.float64(f_swp)
        out["hit_anchors_%d" % n] = np.int32(round(float(r_swp) * K))
        print(n, iters, float(f_def), float(r_def), float(f_swp), float(r_swp))
    np.savez(os.path.join(HERE, "anchor_cluster.npz"), **out)


if __name__ == "__main__":
    main()
