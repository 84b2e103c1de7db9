"""Stand-alone forward of the operator classes in build_utils/layers.py and models.YOLOLayer on torch
NCHW float32 CUDA tensors (the reference's `module(x)` / `module(x, outputs)` surface).  Each call converts to the
channels-last compute layout, runs the same HIP kernels the compiled plan uses, and converts back.  This is the
module-level compatibility surface (no autograd); `models.YOLO.forward` never goes through here.
The input-side passes on the loader's uint8 batches live here too: prepare_images, clahe, cutout, augment_pairs,
resize_pad_pairs.
"""
import ctypes

import torch

from . import lib as L
from . import ops
from .lib import check, load


def _dtype():
    return torch.bfloat16 if torch.is_autocast_enabled() else torch.float32


def _ru(n, a):
    return (n + a - 1) // a * a


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nhwc(x, cpad=None):
    ops._require_cuda(x)
    return ops.to_nhwc(x.float().contiguous(), _dtype(), cpad=cpad)


def concat(tensors):
    """FeatureConcat.forward for several inputs (reference layers.py:44)"""
    dt = _dtype()
    B, _, H, W = tensors[0].shape
    cs = [t.shape[1] for t in tensors]
    buf = torch.zeros((B, H, W, sum(cs)), dtype=dt, device=tensors[0].device)
    c0 = 0
    for t, c in zip(tensors, cs):
        ops._require_cuda(t)
        ops.to_nhwc(t.float().contiguous(), dt, out=buf[..., c0:c0 + c])
        c0 += c
    return ops.to_nchw(buf)


def weighted_fusion(x, others, w, n):
    """WeightedFeatureFusion.forward (reference layers.py:63-85); with mismatched channel counts the sum covers the first
    min(nx, na) channels and the output keeps x's channel count (:78-83)"""
    xd = _nhwc(x)
    weff = None
    if w is not None:
        weff = torch.zeros(n, device=x.device)
        check(load().dyk_wfuse_weights(w.detach().float().contiguous().data_ptr(), weff.data_ptr(), n, _stream()))
    out = xd
    for i, a in enumerate(others):
        ad = _nhwc(a)
        nx, na = xd.shape[3], ad.shape[3]
        C = min(nx, na)
        vec = 16 // xd.element_size()
        if nx != na and (C % vec or abs(nx - na) % vec):
            raise NotImplementedError("WeightedFeatureFusion with channel counts %d / %d that are not whole 16-byte vectors" % (nx, na))
        nxt = torch.empty_like(xd)
        w0 = weff[0:1] if (weff is not None and i == 0) else None
        d = ops.ew_desc(a=out[..., :C], b=ad[..., :C], out=nxt[..., :C], p0=w0, p1=weff[i + 1:i + 2] if weff is not None else None)
        ops.call("dyk_axpby", d)
        if nx > na:                                            # the rest of x passes through (scaled by w[0] on the first term)
            ops.call("dyk_axpby", ops.ew_desc(a=out[..., C:], out=nxt[..., C:], p0=w0))
        out = nxt
    return ops.to_nchw(out)


def squeeze_excitation(x, w1, b1, w2, b2):
    """SqueezeExcitation.forward (reference layers.py:184-190)"""
    xd = _nhwc(x)
    B, H, W, C = xd.shape
    Cs = w1.shape[0]
    pooled = torch.zeros(B, C, device=x.device)
    scale = torch.zeros(B, C, device=x.device)
    ops.call("dyk_se_pool", ops.ew_desc(a=xd, B=B, H=H, W=W, alpha=1.0 / (H * W)), pooled)
    prm = [t.detach().float().contiguous() for t in (w1, b1, w2, b2)]
    fd = L.DykSeFcDesc()
    fd.pooled, fd.scale = pooled.data_ptr(), scale.data_ptr()
    fd.w1, fd.b1, fd.w2, fd.b2 = (t.data_ptr() for t in prm)
    fd.B, fd.C, fd.Cs = B, C, Cs
    fcws = torch.empty(B * (C + 2 * Cs), device=x.device)       # h | dt1 | t2 (include/dyk_hip.h)
    fd.ws = fcws.data_ptr()
    ops.call("dyk_se_fc_fwd", fd)
    z = torch.empty_like(xd)
    ops.call("dyk_se_scale", ops.ew_desc(a=xd, out=z, p0=scale, B=B, H=H, W=W))
    return ops.to_nchw(z)


def conv_bn_act(x, conv, bn, act, training):
    """nn.Sequential(Conv2d[, BatchNorm2d][, activation]) forward (reference models.py:28-64); dense or depthwise."""
    dt = _dtype()
    k, s, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    cin, cout = conv.in_channels, conv.out_channels
    depthwise = conv.groups > 1
    if depthwise and not (conv.groups == cin == cout):
        raise NotImplementedError("grouped convolution that is not depthwise")
    cpad = _ru(cin, 32)
    xd = _nhwc(x, cpad=cpad)
    dev = x.device
    if depthwise:
        if bn is None:
            raise NotImplementedError("depthwise convolution without BatchNorm2d")
        wt = conv.weight.detach().float().reshape(cout, k * k).t().contiguous()

        def run_conv(stats=None, **epi):
            return ops.dwconv_fwd(xd, wt, k, s, pad, stats=stats, stats_slots=1, C=cout)
    else:
        wp = ops.pack_weight(conv.weight.detach().float().contiguous(), dt, cin_pad=cpad)

        def run_conv(stats=None, **epi):
            return ops.conv2d_fwd(xd, wp, k, s, pad, cout, stats=stats, **epi)
    if bn is None:
        bias = conv.bias.detach().float().contiguous() if conv.bias is not None else None
        return ops.to_nchw(run_conv(act=act, shift=bias))
    gamma, beta = bn.weight.detach().float().contiguous(), bn.bias.detach().float().contiguous()
    if not training:
        scale, shift = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
        check(load().dyk_bn_fold(gamma.data_ptr(), beta.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                 float(bn.eps), scale.data_ptr(), shift.data_ptr(), cout, _stream()))
        if not depthwise:
            return ops.to_nchw(run_conv(act=act, scale=scale, shift=shift))
        y = run_conv()
    else:
        stats = torch.zeros(2 * cout, dtype=torch.float64, device=dev)
        y = run_conv(stats=stats)
        n = y.shape[0] * y.shape[1] * y.shape[2]
        scale, shift, _, _ = ops.bn_finalize(stats, n, gamma, beta, bn.running_mean, bn.running_var,
                                             momentum=bn.momentum if bn.momentum is not None else 0.1, eps=bn.eps)
        bn.num_batches_tracked += 1
    z = torch.empty_like(y)
    ops.call("dyk_bn_act_fwd", ops.ew_desc(a=y, out=z, act=act, p0=scale, p1=shift, C=cout))
    return ops.to_nchw(z, C=cout)


def maxpool(x, k, stride=1):
    xd = _nhwc(x)
    B, H, W, C = xd.shape
    z = torch.empty((B, ops.maxpool_out_size(H, k, stride), ops.maxpool_out_size(W, k, stride), C), dtype=xd.dtype, device=xd.device)
    d = ops.ew_desc(a=xd, out=z, B=B, H=H, W=W, k=k)
    d.slots = stride
    ops.call("dyk_maxpool_fwd", d, None)
    return ops.to_nchw(z)


def upsample2x(x):
    xd = _nhwc(x)
    B, H, W, C = xd.shape
    z = torch.empty((B, 2 * H, 2 * W, C), dtype=xd.dtype, device=xd.device)
    ops.call("dyk_upsample2x_fwd", ops.ew_desc(a=xd, out=z, B=B, H=H, W=W))
    return ops.to_nchw(z)


def yolo_layer(p, layer):
    """YOLOLayer.forward (reference models.py:218-258): p [B, na*no, ny, nx] -> training: [B,na,ny,nx,no];
    eval: (decoded [B, na*ny*nx, no], raw)"""
    ops._require_cuda(p)
    B, _, ny, nx = p.shape
    na, no = layer.na, layer.no
    y = torch.zeros((B, ny, nx, 32 if na * no <= 32 else _ru(na * no, 4)), dtype=torch.float32, device=p.device)
    ld = y.shape[3]
    ops.to_nhwc(p.float().contiguous(), torch.float32, out=y[..., :na * no])
    out = torch.empty((B, na, ny, nx, no), dtype=torch.float32, device=p.device)
    check(load().dyk_head_permute_fwd(y.data_ptr(), out.data_ptr(), B, ny, nx, na, no, ld, _stream()))
    if layer.training:
        return out
    io = torch.empty((B, na * ny * nx, no), dtype=torch.float32, device=p.device)
    d = L.DykDecodeDesc()
    d.p, d.io = out.data_ptr(), io.data_ptr()
    d.B, d.na, d.ny, d.nx, d.no = B, na, ny, nx, no
    d.rows_total, d.row_offset, d.v4, d.stride = na * ny * nx, 0, 1 if layer.bf_type == "yolov4" else 0, float(layer.stride)
    for i, v in enumerate(layer.anchor_vec.detach().float().cpu().reshape(-1).tolist()):
        d.anchor_vec[i] = v
    ops.call("dyk_yolo_decode", d)
    return io, out


def prepare_images(imgs, size=None, div=255.0):
    """Harness input path (reference train_utils/kaist_train_eval_utils.py:54-55, 59-71): the loader's uint8 batch
    [B,3,H,W] -> float32 in 0..1, optionally resized like F.interpolate(size=size, mode='bilinear',
    align_corners=False), in one HIP pass.  float32 input is taken as already divided (div forced to 1)."""
    ops._require_cuda(imgs)
    if imgs.dim() != 4:
        raise ValueError("prepare_images expects [B,C,H,W], got %s" % (tuple(imgs.shape),))
    if imgs.dtype == torch.uint8:
        sdt = L.DYK_U8
    elif imgs.dtype == torch.float32:
        sdt, div = L.DYK_F32, 1.0
    else:
        raise TypeError("prepare_images: uint8 or float32 images, got %s" % imgs.dtype)
    imgs = imgs.contiguous()
    B, C, H, W = imgs.shape
    Ho, Wo = (H, W) if size is None else (int(size[0]), int(size[1]))
    out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=imgs.device)
    check(load().dyk_image_prep(imgs.data_ptr(), out.data_ptr(), B * C, H, W, Ho, Wo, sdt, float(div), _stream()),
          "dyk_image_prep")
    return out


def multi_scale_pair(v_imgs, l_imgs, img_size, gs=32):
    """The multi-scale step of the reference training loop (kaist_train_eval_utils.py:59-71): scale factor
    sf = img_size / max(H, W), new size ceil(x*sf/gs)*gs per axis, both streams resized alike."""
    import math
    assert v_imgs.shape[:2] == l_imgs.shape[:2]
    sf = img_size / max(v_imgs.shape[2:])
    ns = None
    if sf != 1:
        ns = [math.ceil(x * sf / gs) * gs for x in v_imgs.shape[2:]]
    return prepare_images(v_imgs, ns), prepare_images(l_imgs, ns)


def _u8_planes(imgs, what):
    if not isinstance(imgs, torch.Tensor):
        raise TypeError("%s: a uint8 device tensor [..., H, W], got %s" % (what, type(imgs).__name__))
    if not imgs.is_cuda:
        raise TypeError("%s runs on the GPU only (got a %s tensor); there is no CPU fallback" % (what, imgs.device.type))
    if imgs.dtype != torch.uint8:
        raise TypeError("%s: uint8 images, got %s" % (what, imgs.dtype))
    if imgs.dim() < 2:
        raise ValueError("%s expects [..., H, W], got %s" % (what, tuple(imgs.shape),))
    if not imgs.is_contiguous():
        raise ValueError("%s: a contiguous tensor (planar [..., H, W])" % what)
    H, W = int(imgs.shape[-2]), int(imgs.shape[-1])
    planes = imgs.numel() // max(H * W, 1)
    if planes < 1 or H < 1 or W < 1:
        raise ValueError("%s: an empty tensor %s" % (what, tuple(imgs.shape),))
    return planes, H, W


def clahe(imgs, clip_limit=1.0, tile_grid_size=(4, 4), out=None):
    """OpenCV's 8-bit CLAHE (cv2.createCLAHE(clipLimit, tileGridSize).apply) on every plane of a uint8 device tensor
    [..., H, W], e.g. the loader's [B,3,H,W]: dyk_clahe, two launches, no synchronisation; the rule is in include/dyk_hip.h.
    `tile_grid_size` is (tiles_x, tiles_y) as in cv2; `out` may be `imgs` itself.  ValueError for what the rule refuses:
    a grid outside 1..16, a pad beyond n - 1 pixels on its axis, a tile above 2^24 pixels."""
    planes, H, W = _u8_planes(imgs, "clahe")
    try:
        tx, ty = (int(t) for t in tile_grid_size)
    except (TypeError, ValueError):
        raise TypeError("clahe: tile_grid_size is (tiles_x, tiles_y), got %r" % (tile_grid_size,))
    if not (1 <= tx <= L.CLAHE_MAX_TILES and 1 <= ty <= L.CLAHE_MAX_TILES):
        raise ValueError("clahe: tile_grid_size within 1..%d per axis, got %r" % (L.CLAHE_MAX_TILES, tile_grid_size))
    padx, pady = (0, 0) if (W % tx == 0 and H % ty == 0) else (tx - W % tx, ty - H % ty)
    if padx > W - 1 or pady > H - 1:
        raise ValueError("clahe: a %dx%d image cannot be padded by (%d, %d) for a %r grid" % (H, W, pady, padx, tile_grid_size))
    if ((W + padx) // tx) * ((H + pady) // ty) > 1 << 24:
        raise ValueError("clahe: tiles of more than 2^24 pixels")
    if out is None:
        out = torch.empty_like(imgs)
    elif _u8_planes(out, "clahe(out=)") != (planes, H, W) or out.shape != imgs.shape or out.device != imgs.device:
        raise ValueError("clahe: out must match imgs, got %s for %s" % (tuple(out.shape), tuple(imgs.shape)))
    lut = torch.empty(load().dyk_clahe_ws_bytes(planes, tx, ty), dtype=torch.uint8, device=imgs.device)
    d = L.DykClaheDesc(src=imgs.data_ptr(), dst=out.data_ptr(), lut=lut.data_ptr(), planes=planes, H=H, W=W, tiles_x=tx,
                       tiles_y=ty, clip_limit=float(clip_limit))
    check(load().dyk_clahe(ctypes.byref(d), _stream()), "dyk_clahe")
    return out


def cutout(imgs, rects, value=0):
    """Set rectangles of a uint8 device tensor [..., C, H, W] to `value`, in place, in one launch (dyk_cutout_rects; the
    cut-outs of build_utils.snowflake).  `rects` int32 (xmin, ymin, xmax, ymax), upper ends exclusive, clipped to the image:
    [nrect,4] for every plane, or [B,nrect,4] with B = imgs.shape[0], one set per image.  A host `rects` goes up in one
    small copy; nothing synchronises."""
    planes, H, W = _u8_planes(imgs, "cutout")
    if not isinstance(rects, torch.Tensor):
        raise TypeError("cutout: rects is an int32 tensor, got %s" % type(rects).__name__)
    if rects.dtype != torch.int32:
        raise TypeError("cutout: int32 rects, got %s" % rects.dtype)
    if rects.dim() == 2 and rects.shape[1] == 4:
        nsets = 1
    elif rects.dim() == 3 and rects.shape[2] == 4 and imgs.dim() >= 3 and rects.shape[0] == imgs.shape[0]:
        nsets = int(rects.shape[0])
    else:
        raise ValueError("cutout: rects [nrect,4] or [%s,nrect,4], got %s" % (imgs.shape[0] if imgs.dim() else "B", tuple(rects.shape)))
    if not 0 <= int(value) <= 255:
        raise ValueError("cutout: value within 0..255, got %r" % (value,))
    nrect = int(rects.shape[-2])
    if nrect == 0:
        return imgs
    rects = rects.contiguous().to(imgs.device, non_blocking=True)
    check(load().dyk_cutout_rects(imgs.data_ptr(), planes, H, W, rects.data_ptr(), nrect, planes // nsets, int(value), _stream()),
          "dyk_cutout_rects")
    return imgs


def invert_affine(M):
    """The inverse of a forward affine matrix (rows 0 and 1 of a 2 x 3 or 3 x 3) as dyk_augment_pairs takes it: six Python
    floats, formed in fp64 in exactly the order of the rule (include/dyk_hip.h, (b)).  ValueError for a non-finite or
    singular matrix."""
    import math
    m = [float(M[0][0]), float(M[0][1]), float(M[0][2]), float(M[1][0]), float(M[1][1]), float(M[1][2])]
    if not all(math.isfinite(t) for t in m):
        raise ValueError("augment_pairs: a non-finite matrix %r" % (m,))
    D = m[0] * m[4] - m[1] * m[3]
    if D == 0.0:
        raise ValueError("augment_pairs: a singular matrix %r" % (m,))
    D = 1.0 / D
    A11 = m[4] * D
    A22 = m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2] = b1
    m[5] = b2
    if not all(math.isfinite(t) for t in m):
        raise ValueError("augment_pairs: the inverse of the matrix is not finite: %r" % (m,))
    return m


def _host_array(a, dtype, shape, what):
    import numpy as np
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise TypeError("augment_pairs: %s is a host array (it goes up with the other parameters in one copy)" % what)
        a = a.numpy()
    a = np.asarray(a)
    if dtype == np.uint8 and a.dtype not in (np.uint8, np.bool_):
        raise TypeError("augment_pairs: %s is uint8, got %s" % (what, a.dtype))
    if dtype == np.int32 and a.dtype.kind not in "iu":
        raise TypeError("augment_pairs: %s holds integers, got %s" % (what, a.dtype))
    if a.ndim != len(shape) or any(s is not None and s != t for s, t in zip(shape, a.shape)):
        raise ValueError("augment_pairs: %s has shape %s, got %s" % (what, ["B" if s is None else s for s in shape], a.shape))
    return np.ascontiguousarray(a.astype(dtype, copy=False))


def augment_pairs(v, l, matrices=None, rects=None, canvas=None, out_size=None, luts=None, flip=None, out=None):
    """Mosaic canvas, affine warp, HSV jitter and left-right flip of image pairs in ONE launch (dyk_augment_pairs,
    csrc/augment.hip; the rule is in include/dyk_hip.h).  `v`, `l`: uint8 device batches [N,3,H,W].  All of the following are
    host arrays, per output image b of B, shared by both streams, and go up in one small copy from pinned memory; nothing
    synchronises:
      matrices [B,2,3] fp64   the FORWARD matrix (source -> output), as cv2.warpAffine takes it; inverted here.  None: identity
      rects    [B,4,8] int32  (x1, y1, x2, y2, src, dx, dy, 0) with canvas=(Hc, Wc): the virtual canvas.  None: image b itself
      out_size (Ho, Wo)       default: the canvas size
      luts     [B,3,256] u8   the hue / saturation / value tables.  None: no jitter
      flip     [B]            non-zero: store mirrored.  None: none
    `out=(ov, ol)`: uint8 [B,3,Ho,Wo]; they may be `v`, `l` themselves only for jitter alone.  -> (ov, ol).
    TypeError / ValueError for what the entry refuses and for the warp limits: a non-finite or singular matrix, a size above
    16384, a matrix that maps an output corner to 2^20 pixels or beyond or moves the source that far across the output, a
    rectangle that reaches outside its source."""
    import numpy as np
    for t, what in ((v, "v"), (l, "l")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("augment_pairs: %s is a uint8 device tensor [N,3,H,W], got %s" % (what, type(t).__name__))
        if not t.is_cuda:
            raise TypeError("augment_pairs runs on the GPU only (got a %s tensor); there is no CPU fallback" % t.device.type)
        if t.dtype != torch.uint8:
            raise TypeError("augment_pairs: uint8 images, got %s" % t.dtype)
        if t.dim() != 4 or t.shape[1] != 3 or not t.is_contiguous() or t.numel() == 0:
            raise ValueError("augment_pairs: %s is a contiguous planar batch [N,3,H,W], got %s" % (what, tuple(t.shape)))
    if v.shape != l.shape or v.device != l.device:
        raise ValueError("augment_pairs: two batches of one shape on one device, got %s and %s" % (tuple(v.shape), tuple(l.shape)))
    N, _, H, W = (int(s) for s in v.shape)
    B = None
    for a in (matrices, rects, luts, flip):
        if a is not None:
            B = len(a)
            break
    B = N if B is None else B
    if B < 1:
        raise ValueError("augment_pairs: an empty batch of parameters")
    if rects is None:
        if canvas is not None and tuple(canvas) != (H, W):
            raise ValueError("augment_pairs: canvas= belongs to rects=; without them the canvas is the image, %r" % ((H, W),))
        if B != N:
            raise ValueError("augment_pairs: %d parameter sets for %d images; only rects= can pick sources" % (B, N))
        Hc, Wc = H, W
    else:
        if canvas is None:
            raise ValueError("augment_pairs: rects= needs canvas=(Hc, Wc)")
        Hc, Wc = (int(s) for s in canvas)
    Ho, Wo = (Hc, Wc) if out_size is None else (int(s) for s in out_size)
    sizes = (N, B, H, W, Hc, Wc, Ho, Wo)
    if min(sizes) < 1 or max(sizes) > L.AUGMENT_MAX_SIZE:
        raise ValueError("augment_pairs: every size within 1..%d, got N, B, H, W, Hc, Wc, Ho, Wo = %r" % (L.AUGMENT_MAX_SIZE, sizes))
    if matrices is None and (Ho, Wo) != (Hc, Wc):
        raise ValueError("augment_pairs: out_size %r differs from the canvas %r and there is no matrix" % ((Ho, Wo), (Hc, Wc)))

    parts, offs, nbytes = {}, {}, 0
    if matrices is not None:
        M = _host_array(matrices, np.float64, (B, 2, 3), "matrices")
        minv = np.empty((B, 6), np.float64)
        for b in range(B):
            m = minv[b] = invert_affine(M[b])
            for x, y in ((0, 0), (Wo - 1, 0), (0, Ho - 1), (Wo - 1, Ho - 1)):
                if not (abs(m[0] * x + m[1] * y + m[2]) < 2.0 ** 20 and abs(m[3] * x + m[4] * y + m[5]) < 2.0 ** 20):
                    raise ValueError("augment_pairs: matrix %d maps the output corner (%d, %d) 2^20 pixels away or more" % (b, x, y))
            # the column and row terms on their own (ad, bd, X0, Y0 of the rule): with these below 2^20 no rn saturates
            if not max(abs(m[0] * (Wo - 1)), abs(m[3] * (Wo - 1)), abs(m[1] * (Ho - 1)), abs(m[4] * (Ho - 1))) < 2.0 ** 20:
                raise ValueError("augment_pairs: matrix %d moves the source by 2^20 pixels or more across the output" % b)
        parts["minv"] = minv
    if rects is not None:
        R = _host_array(rects, np.int32, (B, 4, 8), "rects")
        for b in range(B):
            for x1, y1, x2, y2, s, dx, dy, _pad in R[b].tolist():
                x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, Wc), min(y2, Hc)
                if x2 <= x1 or y2 <= y1:
                    continue                                     # an unused slot
                if not (0 <= s < N and x1 - dx >= 0 and x2 - dx <= W and y1 - dy >= 0 and y2 - dy <= H):
                    raise ValueError("augment_pairs: rectangle %r of image %d reaches outside source %d of %d x %d"
                                     % ((x1, y1, x2, y2, dx, dy), b, s, H, W))
        parts["rects"] = R
    if luts is not None:
        parts["luts"] = _host_array(luts, np.uint8, (B, 3, 256), "luts")
    if flip is not None:
        parts["flip"] = _host_array(np.asarray(flip.numpy() if isinstance(flip, torch.Tensor) else flip).astype(bool), np.uint8, (B,), "flip")

    if out is None:
        ov = torch.empty((B, 3, Ho, Wo), dtype=torch.uint8, device=v.device)
        ol = torch.empty_like(ov)
    else:
        ov, ol = out
        for t in (ov, ol):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != v.device:
                raise TypeError("augment_pairs: out=(ov, ol), uint8 tensors on the device of the images")
            if tuple(t.shape) != (B, 3, Ho, Wo) or not t.is_contiguous():
                raise ValueError("augment_pairs: out tensors are contiguous %r, got %s" % ((B, 3, Ho, Wo), tuple(t.shape)))

    ptr = dict.fromkeys(("minv", "rects", "luts", "flip"))
    if parts:
        for k in ("minv", "rects", "luts", "flip"):              # fp64 first, then int32, then bytes: every part aligned
            if k in parts:
                offs[k] = nbytes
                nbytes += parts[k].nbytes
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        for k, o in offs.items():
            hv[o:o + parts[k].nbytes] = parts[k].reshape(-1).view(np.uint8)
        dev = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
        dev.copy_(host, non_blocking=True)
        for k, o in offs.items():
            ptr[k] = dev.data_ptr() + o
    d = L.DykAugmentDesc(src_v=v.data_ptr(), src_l=l.data_ptr(), dst_v=ov.data_ptr(), dst_l=ol.data_ptr(), N=N, B=B, H=H, W=W,
                         Hc=Hc, Wc=Wc, Ho=Ho, Wo=Wo, rects=ptr["rects"], minv=ptr["minv"], luts=ptr["luts"], flip=ptr["flip"])
    rc = load().dyk_augment_pairs(ctypes.byref(d), _stream())
    if rc == -1:
        raise ValueError("augment_pairs: dyk_augment_pairs refused the call (out tensors that overlap the inputs, or each other? "
                         "only jitter alone may run in place)")
    check(rc, "dyk_augment_pairs")
    return ov, ol


RESIZE_LINEAR, RESIZE_AREA = 0, 1
_LAYOUTS = {"chw": 0, "hwc_bgr": 1}


def _image_list(t, what, layout):
    """a batch tensor or a list of per-image tensors -> [(tensor, h, w)], every one a contiguous uint8 device image"""
    imgs = list(t.unbind(0)) if isinstance(t, torch.Tensor) else list(t)
    out = []
    for i, im in enumerate(imgs):
        if not isinstance(im, torch.Tensor):
            raise TypeError("resize_pad_pairs: %s[%d] is a uint8 device tensor, got %s" % (what, i, type(im).__name__))
        if not im.is_cuda:
            raise TypeError("resize_pad_pairs runs on the GPU only (%s[%d] is a %s tensor); there is no CPU fallback" % (what, i, im.device.type))
        if im.dtype != torch.uint8:
            raise TypeError("resize_pad_pairs: uint8 images, got %s for %s[%d]" % (im.dtype, what, i))
        ch = 0 if layout == "chw" else 2
        if im.dim() != 3 or im.shape[ch] != 3 or not im.is_contiguous() or im.numel() == 0:
            raise ValueError("resize_pad_pairs: %s[%d] is a contiguous %s image, got %s" % (what, i, "[3,h,w]" if layout == "chw" else "[h,w,3]", tuple(im.shape)))
        h, w = (int(im.shape[1]), int(im.shape[2])) if layout == "chw" else (int(im.shape[0]), int(im.shape[1]))
        out.append((im, h, w))
    return out


def resize_pad_pairs(v_list, l_list, geom, out_size, layout="chw", color=(0, 0, 0), out=None):
    """Resize (LINEAR / AREA) and letterbox of image pairs in ONE launch (dyk_resize_pad_pairs, csrc/letterbox.hip; the rule is
    in include/dyk_hip.h).  `v_list`, `l_list`: a uint8 device batch [B,3,h,w] (layout "chw") or [B,h,w,3] (layout "hwc_bgr":
    cv2.imread's array, the channels reversed on the way so that the output is planar RGB), or lists of B per-image tensors,
    which may differ in size from image to image (not between the two streams).  `geom`: per image (nh, nw, top, left, interp)
    on the host -- the resized content size, its place in the output, RESIZE_LINEAR (0) or RESIZE_AREA (1); both streams share
    it.  `out_size` (Ho, Wo); `color` the border value per output plane; `out=(ov, ol)` uint8 [B,3,Ho,Wo].  The records and
    source addresses go up in one small copy from pinned memory; nothing synchronises.  -> (ov, ol).
    TypeError / ValueError for everything the entry refuses (sizes outside 1..16384, a content rectangle outside the output, AREA
    that would enlarge, overlapping tensors) and for non-uint8, non-contiguous or host tensors."""
    import numpy as np
    if layout not in _LAYOUTS:
        raise ValueError("resize_pad_pairs: layout is 'chw' or 'hwc_bgr', got %r" % (layout,))
    vs, ls = _image_list(v_list, "v_list", layout), _image_list(l_list, "l_list", layout)
    B = len(vs)
    if B < 1 or len(ls) != B or len(geom) != B:
        raise ValueError("resize_pad_pairs: %d visible images, %d LWIR images and %d geometry records" % (B, len(ls), len(geom)))
    Ho, Wo = (int(s) for s in out_size)
    color = [int(c) for c in (color if hasattr(color, "__len__") else (color,) * 3)]
    if len(color) != 3 or min(color) < 0 or max(color) > 255:
        raise ValueError("resize_pad_pairs: color is three values of 0..255, got %r" % (color,))
    M = L.RESIZE_PAD_MAX_SIZE
    if not (1 <= B <= M and 1 <= Ho <= M and 1 <= Wo <= M):
        raise ValueError("resize_pad_pairs: B, Ho, Wo within 1..%d, got %r" % (M, (B, Ho, Wo)))
    dev = vs[0][0].device
    recs = (L.DykResizePadRec * B)()
    for b, ((v, h, w), (l, hl, wl)) in enumerate(zip(vs, ls)):
        if (h, w) != (hl, wl) or v.device != dev or l.device != dev:
            raise ValueError("resize_pad_pairs: image %d: the two streams have one size and one device, got %s and %s" % (b, tuple(v.shape), tuple(l.shape)))
        nh, nw, top, left, interp = (int(t) for t in geom[b])
        if not (1 <= h <= M and 1 <= w <= M and 1 <= nh <= M and 1 <= nw <= M):
            raise ValueError("resize_pad_pairs: image %d: sizes within 1..%d, got %r -> %r" % (b, M, (h, w), (nh, nw)))
        if interp not in (RESIZE_LINEAR, RESIZE_AREA):
            raise ValueError("resize_pad_pairs: image %d: interp is RESIZE_LINEAR (0) or RESIZE_AREA (1), got %r" % (b, interp))
        if top < 0 or left < 0 or top + nh > Ho or left + nw > Wo:
            raise ValueError("resize_pad_pairs: image %d: content %d x %d at (%d, %d) does not lie inside the output %d x %d" % (b, nh, nw, top, left, Ho, Wo))
        if interp == RESIZE_AREA and (nh > h or nw > w):
            raise ValueError("resize_pad_pairs: image %d: AREA does not enlarge (%r -> %r)" % (b, (h, w), (nh, nw)))
        recs[b] = L.DykResizePadRec(src_v=v.data_ptr(), src_l=l.data_ptr(), h=h, w=w, nh=nh, nw=nw, top=top, left=left, interp=interp)
    if out is None:
        ov = torch.empty((B, 3, Ho, Wo), dtype=torch.uint8, device=dev)
        ol = torch.empty_like(ov)
    else:
        ov, ol = out
        for t in (ov, ol):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != dev:
                raise TypeError("resize_pad_pairs: out=(ov, ol), uint8 tensors on the device of the images")
            if tuple(t.shape) != (B, 3, Ho, Wo) or not t.is_contiguous():
                raise ValueError("resize_pad_pairs: out tensors are contiguous %r, got %s" % ((B, 3, Ho, Wo), tuple(t.shape)))
    nbytes = ctypes.sizeof(recs)
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = np.frombuffer(recs, dtype=np.uint8)
    drecs = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    drecs.copy_(host, non_blocking=True)
    d = L.DykResizePadDesc(recs=drecs.data_ptr(), recs_host=ctypes.addressof(recs), dst_v=ov.data_ptr(), dst_l=ol.data_ptr(), B=B, Ho=Ho,
                           Wo=Wo, layout=_LAYOUTS[layout], color=(ctypes.c_uint8 * 3)(*color))
    rc = load().dyk_resize_pad_pairs(ctypes.byref(d), _stream())
    if rc == -1:
        raise ValueError("resize_pad_pairs: dyk_resize_pad_pairs refused the call (out tensors that overlap each other or an input?)")
    check(rc, "dyk_resize_pad_pairs")
    return ov, ol
