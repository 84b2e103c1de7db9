"""Anchor clustering for a new label set -- the reference's other_utils/anchor_cluster.py (wh_iou :153, k_means :169,
anchor_fitness :199, anchor_cluster :219, change_cfg_file_anchors :273, the two label readers) with every N-sized pass on the
device: dyk_anchor_assign, dyk_anchor_median and dyk_anchor_fitness (csrc/anchors.hip; the rule is in include/dyk_hip.h and
restated in tests/anchor_ref.py).  The host keeps what is small and sequential: the label readers, the random draws (so that
seeding `random` and `np.random` reproduces the reference's initial centres and mutation factors draw for draw) and the
accept decisions.  There is no CPU fallback: the compute functions raise dyk.lib.DykLibraryError when libdyk_hip.so is missing
and need a GPU; importing this module, the readers, `wh_iou`, `draw_factors` and `change_cfg_file_anchors`' file handling do
not.

Named departures from the reference:
  * fitness orientation.  The reference calls `anchor_fitness(k, wh, thr)` against the definition `anchor_fitness(whs,
    anchors, thr)`: as called, the value is the mean over the anchors of each anchor's best-matching box, which is close to 1
    whatever the anchors are, so its genetic stage optimises almost nothing.  `fitness="boxes"` (the default) scores what the
    docstring intends, the mean over the boxes of each box's best anchor; `fitness="reference"` reproduces the swapped call.
  * fp64 fitness throughout.  The reference computes its starting fitness from the fp32 k-means centres in fp32 and every
    later one in fp64; here the starting value and the evolution both use the fp64 rule.
  * empty clusters.  A cluster that loses all members keeps its centre (np.median of nothing is NaN in the reference, after
    which np.argmin sends every box to that cluster); `k_means` warns once per call and names the cluster.
  * the `best recall` printed after the genetic stage is that of the returned anchors, not of the last generation's candidate.
  * `fitness="reference"` adds the K per-anchor values in anchor order; the reference's `mean` adds them pairwise, so the two
    agree to within the rounding of a sum of K terms (2 K 2^-53 relative), not always bit for bit.
  * the readers are more forgiving in two places: `VOCDatasetLabels.get_info` skips an annotation without any `object` (the
    reference raises KeyError), and `YOLODatasetLabels` reads an empty label file as zero rows of five columns (the reference
    keeps a 1-D empty array, on which its `get_info` fails).
Additions to the reference's surface, kept small: `evolve_anchors` (the issue's), `draw_factors` and `fitness_batch` (the two
halves of it, which the tests and the probe call), `k_means(init=)`, and `info=` on `k_means` / `evolve_anchors`, a dict that
receives the call's launch and read-back counts.
Evolution is batched without changing its result: the mutation draws never look at a fitness, so all of them are drawn first;
`window` candidates of the current anchors are scored in ONE launch and the first one that beats the current fitness is taken,
which is the sequential chain's decision for every `window`.
"""
import os
import random
import warnings

import numpy as np

FITNESS_KINDS = ("boxes", "reference")


# ------------------------------------------------------------------------------------------------ host: label readers
def _progress(it, desc):
    try:
        from tqdm import tqdm
    except ImportError:
        return it
    return tqdm(it, desc=desc)


def exif_size(img):
    """(w, h) of a PIL image, swapped when the EXIF orientation says the picture lies on its side"""
    s = img.size
    try:
        from PIL import ExifTags
        key = [k for k, v in ExifTags.TAGS.items() if v == "Orientation"][0]
        if dict(img._getexif().items())[key] in (6, 8):
            s = (s[1], s[0])
    except Exception:
        pass
    return s


class VOCDatasetLabels(object):
    """Image sizes and normalised box sizes from a VOC tree: root/Annotations/*.xml named by root/ImageSets/Main/<txt_name>"""

    def __init__(self, root_path, txt_name="test.txt"):
        assert os.path.exists(root_path), "VOC Dataset not exist at {}".format(root_path)
        self.annotations_root_path = os.path.join(root_path, "Annotations")
        txt = os.path.join(root_path, "ImageSets", "Main", txt_name)
        assert os.path.exists(txt), "not found txt file {}".format(txt_name)
        with open(txt, "r") as f:
            self.xml_list = [os.path.join(self.annotations_root_path, ln.strip() + ".xml") for ln in f if ln.strip()]
        assert len(self.xml_list) > 0, "in '{}' file does not find any information".format(txt_name)
        for p in self.xml_list:
            assert os.path.exists(p), "not found '{}' file".format(p)

    def __len__(self):
        return len(self.xml_list)

    def parse_xml_to_dict(self, xml):
        """an element tree as nested dicts; `object` children collect into a list"""
        if len(xml) == 0:
            return {xml.tag: xml.text}
        out = {}
        for child in xml:
            sub = self.parse_xml_to_dict(child)
            if child.tag == "object":
                out.setdefault("object", []).append(sub["object"])
            else:
                out[child.tag] = sub[child.tag]
        return {xml.tag: out}

    def get_info(self):
        """-> ([[W, H] per image with boxes], [[[w / W, h / H] per box] per such image])"""
        import xml.etree.ElementTree as ET
        im_wh, boxes_wh = [], []
        for p in _progress(self.xml_list, "read voc wh info."):
            with open(p) as f:
                data = self.parse_xml_to_dict(ET.fromstring(f.read()))["annotation"]
            H, W = int(data["size"]["height"]), int(data["size"]["width"])
            wh = []
            for obj in data.get("object", []):
                bb = obj["bndbox"]
                wh.append([(float(bb["xmax"]) - float(bb["xmin"])) / W, (float(bb["ymax"]) - float(bb["ymin"])) / H])
            if wh:
                im_wh.append([W, H])
                boxes_wh.append(wh)
        return im_wh, boxes_wh


class YOLODatasetLabels(object):
    """Image sizes and label rows of a YOLO list file: one image path per line, labels beside them (images -> labels,
    jpg -> txt), sizes from the `.shapes` file beside the list, which is written when it is missing."""

    def __init__(self, train_data_txt="data/kaist_train_data.txt"):
        try:
            with open(train_data_txt, "r") as f:
                img_files = f.read().splitlines()
        except Exception as e:
            raise FileNotFoundError("Error loading data from '{}': {}".format(train_data_txt, e))
        self.img_files = [p.replace(".jpg", "_visible.jpg") for p in img_files]
        self.label_files = [p.replace("images", "labels").replace("jpg", "txt") for p in img_files]
        n = len(img_files)
        shapes_path = train_data_txt.replace(".txt", ".shapes")
        try:
            with open(shapes_path, "r") as f:
                sp = [x.split() for x in f.read().splitlines()]
        except Exception:
            from PIL import Image
            sp = [exif_size(Image.open(p)) for p in _progress(self.img_files, "reading image shapes")]
            np.savetxt(shapes_path, sp, fmt="%g")
        self.img_shapes = np.array(sp, dtype=np.float64)
        self.labels = [np.zeros((0, 5), dtype=np.float32)] * n
        for i, p in enumerate(_progress(self.label_files, "Caching labels")):
            try:
                with open(p, "r") as f:
                    self.labels[i] = np.array([x.split() for x in f.read().splitlines()], dtype=np.float32).reshape(-1, 5)
            except Exception as e:
                print("An error occurred while loading the file {}: {}".format(p, e))

    def __len__(self):
        return len(self.labels)

    def get_info(self):
        return self.img_shapes, [b[:, 3:] for b in self.labels]


# ------------------------------------------------------------------------------------------------ host: small pieces
def wh_iou(wh1, wh2):
    """[N,2] x [M,2] -> the [N,M] IoU of boxes that share a corner (host numpy)"""
    a, b = wh1[:, None], wh2[None]
    inter = np.minimum(a, b).prod(2)
    return inter / (a.prod(2) + b.prod(2) - inter)


def draw_factors(shape, gen, mp=0.9, sigma=0.1):
    """The mutation factors of `gen` generations, drawn from np.random and random in the reference's order (a uniform mask
    array, one scalar, a normal array; redrawn while every factor is 1).  -> fp64 [gen, *shape]"""
    npr = np.random
    out = np.empty((gen,) + tuple(shape), dtype=np.float64)
    for g in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            mask = npr.random(shape) < mp
            scale = random.random()
            noise = npr.randn(*shape)
            v = (mask * scale * noise * sigma + 1).clip(0.3, 3.0)
        out[g] = v
    return out


# ------------------------------------------------------------------------------------------------ device plumbing
def _torch():
    import torch
    return torch


def _is_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _device_boxes(wh, what="boxes", check=True):
    """numpy [N,2] or a device tensor [N,2], fp32 | fp64, contiguous -> (device tensor, elem_bytes).  numpy input is checked
    for finite values > 0 on the host; a device tensor is checked by one assignment launch against a single centre, which
    counts the bad rows (check=False: the caller's own first assignment does that)."""
    from dyk import lib as L
    torch = _torch()
    if _is_tensor(wh):
        if not wh.is_cuda:
            raise TypeError("anchor_cluster: %s is a numpy array or a device tensor; there is no CPU fallback for %s tensors" % (what, wh.device.type))
        if wh.dtype not in (torch.float32, torch.float64):
            raise TypeError("anchor_cluster: %s is fp32 or fp64, got %s" % (what, wh.dtype))
        contiguous = wh.is_contiguous()
    elif isinstance(wh, np.ndarray):
        if wh.dtype not in (np.float32, np.float64):
            raise TypeError("anchor_cluster: %s is fp32 or fp64, got %s" % (what, wh.dtype))
        contiguous = wh.flags["C_CONTIGUOUS"]
    else:
        raise TypeError("anchor_cluster: %s is a numpy array or a device tensor, got %s" % (what, type(wh).__name__))
    if wh.ndim != 2 or wh.shape[1] != 2 or not contiguous:
        raise ValueError("anchor_cluster: %s is a contiguous [N, 2] array, got shape %s" % (what, tuple(wh.shape)))
    if not 1 <= wh.shape[0] <= L.ANCHOR_MAX_N:
        raise ValueError("anchor_cluster: 1 <= N < 2^27 %s, got %d" % (what, wh.shape[0]))
    if isinstance(wh, np.ndarray):
        if not (np.isfinite(wh).all() and (wh > 0).all()):
            raise ValueError("anchor_cluster: every one of the %s is finite and > 0" % what)
        wh = torch.from_numpy(wh).cuda()
    elif check:
        import ctypes
        lib = L.load()
        N = wh.shape[0]
        c = torch.ones((1, 2), dtype=wh.dtype, device=wh.device)
        nearest = torch.zeros(N, dtype=torch.int32, device=wh.device)
        stats = torch.empty(3, dtype=torch.int32, device=wh.device)
        d = L.DykAnchorAssignDesc(wh=wh.data_ptr(), c=c.data_ptr(), nearest=nearest.data_ptr(), stats=stats.data_ptr(), N=N, K=1,
                                  elem_bytes=wh.element_size())
        L.check(lib.dyk_anchor_assign(ctypes.byref(d), _stream()), "dyk_anchor_assign")
        bad = int(stats[2].item())
        if bad:
            raise ValueError("anchor_cluster: %d of the %d %s are not finite and > 0" % (bad, N, what))
    return wh, wh.element_size()


def _stream():
    import ctypes
    return ctypes.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _anchors64(a, K=None):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if _is_tensor(a) else a, dtype=np.float64)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[2] != 2:
        raise ValueError("anchor_cluster: anchors are [K, 2] or [G, K, 2], got shape %s" % (a.shape,))
    from dyk import lib as L
    if not 1 <= a.shape[1] <= L.ANCHOR_MAX_K:
        raise ValueError("anchor_cluster: 1 <= K <= %d anchors, got %d" % (L.ANCHOR_MAX_K, a.shape[1]))
    if not 1 <= a.shape[0] <= L.ANCHOR_MAX_G:
        raise ValueError("anchor_cluster: 1 <= G <= %d candidates, got %d" % (L.ANCHOR_MAX_G, a.shape[0]))
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError("anchor_cluster: every anchor is finite and > 0")
    return a


def fitness_batch(wh, anchors, thr):
    """Both orientations of the fitness for G candidates in ONE dyk_anchor_fitness call and one read-back.
    wh: boxes (numpy or device tensor); anchors [G,K,2] (or [K,2]); -> dict of numpy arrays fit_boxes, fit_anchors (fp64 [G]),
    hit_boxes, hit_anchors (int32 [G])."""
    import ctypes
    from dyk import lib as L
    lib = L.load()
    torch = _torch()
    dwh, eb = wh if isinstance(wh, tuple) else _device_boxes(wh)
    a = _anchors64(anchors)
    thr = float(thr)
    if not np.isfinite(thr):
        raise ValueError("anchor_cluster: thr is finite, got %r" % thr)
    G, K, N = a.shape[0], a.shape[1], dwh.shape[0]
    da = torch.from_numpy(a).to(dwh.device)
    need = lib.dyk_anchor_fitness_ws_bytes(N, G, K)
    ws = torch.empty(need, dtype=torch.uint8, device=dwh.device)
    out = torch.empty(24 * G, dtype=torch.uint8, device=dwh.device)      # fit_boxes | fit_anchors | hit_boxes | hit_anchors
    p = out.data_ptr()
    d = L.DykAnchorFitnessDesc(wh=dwh.data_ptr(), a=da.data_ptr(), ws=ws.data_ptr(), fit_boxes=p, fit_anchors=p + 8 * G, hit_boxes=p + 16 * G,
                               hit_anchors=p + 20 * G, ws_bytes=need, thr=thr, N=N, K=K, G=G, elem_bytes=eb)
    L.check(lib.dyk_anchor_fitness(ctypes.byref(d), _stream()), "dyk_anchor_fitness")
    host = out.cpu().numpy()
    return {"fit_boxes": host[:8 * G].view(np.float64).copy(), "fit_anchors": host[8 * G:16 * G].view(np.float64).copy(),
            "hit_boxes": host[16 * G:20 * G].view(np.int32).copy(), "hit_anchors": host[20 * G:].view(np.int32).copy()}


def _score(res, kind, N, K):
    """-> (fitness [G], recall [G]) of one orientation"""
    if kind == "boxes":
        return res["fit_boxes"], res["hit_boxes"] / float(N)
    return res["fit_anchors"], res["hit_anchors"] / float(K)


# ------------------------------------------------------------------------------------------------ the reference's surface
def k_means(boxes, k, dist=np.median, init=None, info=None):
    """IoU k-means with median centres, the reference's loop: k distinct boxes drawn with np.random.choice on the host as the
    initial centres (or `init` [k,2], an addition to the reference's signature: nothing is drawn then), then {assign, stop
    when no box changed its cluster, median} on the device (dyk_anchor_assign, dyk_anchor_median; one read-back of the K + 2 counters per iteration).  The assignment buffer starts as zeros, as the
    reference's `last_nearest`, so a first pass that puts every box into cluster 0 returns the initial centres.  A cluster
    that empties keeps its centre (a warning names it).  numpy in -> numpy out, device tensor in -> tensor out, dtype kept.
    `info`: a dict that receives entry_calls, readbacks and iterations."""
    if dist is not np.median:
        raise NotImplementedError("k_means: only dist=np.median is implemented on the device (the reference's default); "
                                  "got %r" % (dist,))
    import ctypes
    from dyk import lib as L
    lib = L.load()
    torch = _torch()
    K = int(k)
    if not 1 <= K <= L.ANCHOR_MAX_K:
        raise ValueError("k_means: 1 <= k <= %d, got %d" % (L.ANCHOR_MAX_K, K))
    dwh, eb = _device_boxes(boxes, check=False)
    N = dwh.shape[0]
    if K > N:
        raise ValueError("k_means: k = %d clusters need at least as many boxes, got %d" % (K, N))
    if init is None:
        idx = np.random.choice(N, K, replace=False)
        c = dwh[torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dwh.device)].contiguous()
    else:
        c = _device_boxes(init, "initial centres")[0].clone()
        if c.shape[0] != K or c.dtype != dwh.dtype or c.device != dwh.device:
            raise ValueError("k_means: init is [k, 2] in the type and on the device of the boxes")
    nearest = torch.zeros(N, dtype=torch.int32, device=dwh.device)
    stats = torch.empty(K + 2, dtype=torch.int32, device=dwh.device)
    da = L.DykAnchorAssignDesc(wh=dwh.data_ptr(), c=c.data_ptr(), nearest=nearest.data_ptr(), stats=stats.data_ptr(), N=N, K=K, elem_bytes=eb)
    ws = torch.empty(lib.dyk_anchor_median_ws_bytes(K), dtype=torch.uint8, device=dwh.device)
    dm = L.DykAnchorMedianDesc(wh=dwh.data_ptr(), nearest=nearest.data_ptr(), c=c.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel(), N=N, K=K, elem_bytes=eb)
    st = _stream()
    empties, calls, readbacks = [], 0, 0
    while True:
        L.check(lib.dyk_anchor_assign(ctypes.byref(da), st), "dyk_anchor_assign")
        s = stats.cpu().numpy()
        calls, readbacks = calls + 1, readbacks + 1
        if s[K + 1]:
            raise ValueError("k_means: %d of the %d boxes are not finite and > 0" % (s[K + 1], N))
        if s[K] == 0:
            break
        for j in np.nonzero(s[:K] == 0)[0]:
            if int(j) not in empties:
                empties.append(int(j))
        L.check(lib.dyk_anchor_median(ctypes.byref(dm), st), "dyk_anchor_median")
        calls += 1
    if empties:
        warnings.warn("k_means: cluster%s %s had no member in some iteration and kept the centre it had (the reference's "
                      "np.median gives NaN there)" % ("s" if len(empties) > 1 else "", ", ".join(str(j) for j in empties)))
    if info is not None:
        info.update(entry_calls=calls, readbacks=readbacks, iterations=readbacks)
    return c if _is_tensor(boxes) else c.cpu().numpy()


def anchor_fitness(whs, anchors, thr):
    """-> (fitness, best_recall) of `anchors` [K,2] over the boxes `whs` [N,2], arguments as named: the mean over the boxes of
    each box's best min(ratio, 1 / ratio), counting only values > thr, and the fraction of boxes above thr.  One launch, G = 1."""
    dwh = _device_boxes(whs)
    a = _anchors64(anchors)
    if a.shape[0] != 1:
        raise ValueError("anchor_fitness: anchors are [K, 2], got shape %s" % (a.shape,))
    res = fitness_batch(dwh, a, thr)
    return res["fit_boxes"][0], res["hit_boxes"][0] / float(dwh[0].shape[0])


def evolve_anchors(wh, k, thr=0.25, gen=1000, fitness="boxes", window=64, mp=0.9, sigma=0.1, info=None):
    """The reference's genetic stage from the anchors `k` [K,2]: generation g multiplies the current anchors by its factors,
    clips at 2.0 and is accepted iff its fitness is > the current one.  All factors are drawn first (draw_factors), then
    `window` consecutive generations of the CURRENT anchors are scored per launch and the first improving one is accepted:
    the sequential chain's result for every window.  `info`: a dict that receives launches, readbacks and accepted.
    -> (anchors fp64 [K,2], fitness, accepted generations)"""
    from dyk import lib as L
    if fitness not in FITNESS_KINDS:
        raise ValueError("evolve_anchors: fitness is 'boxes' or 'reference', got %r" % (fitness,))
    window, gen = int(window), int(gen)
    if not 1 <= window <= L.ANCHOR_MAX_G:
        raise ValueError("evolve_anchors: 1 <= window <= %d, got %d" % (L.ANCHOR_MAX_G, window))
    if gen < 0:
        raise ValueError("evolve_anchors: gen >= 0, got %d" % gen)
    dwh = wh if isinstance(wh, tuple) else _device_boxes(wh)
    k = _anchors64(k)[0].copy()
    N, K = dwh[0].shape[0], k.shape[0]
    f = _score(fitness_batch(dwh, k, thr), fitness, N, K)[0][0]
    v = draw_factors(k.shape, gen, mp, sigma)
    g0, accepted, launches = 0, 0, 1
    while g0 < gen:
        n = min(window, gen - g0)
        cand = (k[None] * v[g0:g0 + n]).clip(min=2.0)
        fg = _score(fitness_batch(dwh, cand, thr), fitness, N, K)[0]
        launches += 1
        better = np.nonzero(fg > f)[0]
        if len(better):
            j = int(better[0])
            f, k = fg[j], cand[j].copy()
            accepted += 1
            g0 += j + 1
        else:
            g0 += n
    if info is not None:
        info.update(launches=launches, readbacks=launches, accepted=accepted)
    return k, f, accepted


def anchor_cluster(img_size=512, n=9, thr=0.25, gen=1000, train_data_txt="data/kaist_train_data.txt", wh=None, fitness="boxes",
                   verbose=True):
    """The reference's sequence: boxes scaled so that the longer image side is `img_size`, a warning for boxes under 3 pixels,
    boxes with both sides under 2 pixels dropped, k_means, sorted by area, evolve_anchors, sorted by area.  `wh` passes boxes
    directly, already scaled (numpy or device tensor).  -> the anchors, fp64 [n,2]"""
    if fitness not in FITNESS_KINDS:
        raise ValueError("anchor_cluster: fitness is 'boxes' or 'reference', got %r" % (fitness,))
    say = print if verbose else (lambda *a: None)
    if wh is None:
        im_wh, boxes_wh = YOLODatasetLabels(train_data_txt=train_data_txt).get_info()
        im_wh = np.array(im_wh, dtype=np.float32)
        shapes = img_size * im_wh / im_wh.max(1, keepdims=True)
        wh0 = np.concatenate([l * s for s, l in zip(shapes, boxes_wh)])
    else:
        wh0 = wh
    small = int((wh0 < 3.0).any(1).sum())
    if small:
        say("WARNING: Extremely small objects found. %d of %d labels are < 3 pixels in size." % (small, len(wh0)))
    wh1 = wh0[(wh0 >= 2.0).any(1)]
    wh1 = wh1.contiguous() if _is_tensor(wh1) else np.ascontiguousarray(wh1)
    k = k_means(wh1, n)
    k = np.asarray(k.cpu().numpy() if _is_tensor(k) else k)
    k = k[np.argsort(k.prod(1))]
    dwh = _device_boxes(wh1, check=False)                # k_means' first assignment has counted the bad rows
    N = dwh[0].shape[0]
    f0, r0 = _score(fitness_batch(dwh, k, thr), fitness, N, n)
    say("kmeans: " + " ".join("[%d, %d]" % (int(a[0]), int(a[1])) for a in k))
    say("fitness: %.5f, best recall: %.5f" % (f0[0], r0[0]))
    k, f, _ = evolve_anchors(dwh, k, thr=thr, gen=gen, fitness=fitness)
    k = k[np.argsort(k.prod(1))]
    r = _score(fitness_batch(dwh, k, thr), fitness, N, n)[1][0]
    say("genetic: " + " ".join("[%d, %d]" % (int(a[0]), int(a[1])) for a in k))
    say("fitness: %.5f, best recall: %.5f" % (f, r))
    return k


def change_cfg_file_anchors(cfg_path, **kw):
    """Clusters (anchor_cluster(**kw)) and rewrites every line of `cfg_path` that starts with `anchors`"""
    k = anchor_cluster(**kw)
    with open(cfg_path, "r") as f:
        lines = f.read().splitlines()
    new = "anchors = " + ", ".join("%d, %d" % (int(a[0]), int(a[1])) for a in k)
    lines = [new if ln.startswith("anchors") else ln for ln in lines]
    with open(cfg_path, "w") as f:
        f.write("\n".join(lines))
    return k


if __name__ == "__main__":
    anchor_cluster()
