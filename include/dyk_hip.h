/*
 * dyk_hip.h -- C ABI of libdyk_hip.so, the MI355X (gfx950) native layer under the
 * Double-YOLO-Kaist Python operator surface.
 *
 * The reference (Ye-zixiao/Double-YOLO-Kaist) has no FFI of its own: its hot path is
 * Python calling torch.nn / torchvision ops.  Every entry point below therefore
 * replaces one *torch call site* of the reference; the call site is cited next to
 * each declaration (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless the
 *     name ends in _host.  No allocation, no synchronisation, no ownership transfer:
 *     buffers are borrowed for the duration of the enqueued work.
 *   - `stream` is a hipStream_t passed as void*; work is enqueued on it and the call
 *     returns immediately.
 *   - return value: 0 on success, negative DYK_ERR_* otherwise.  Nothing throws,
 *     nothing calls exit().
 *   - activations are channels-last: element (b, y, x, c) of a tensor lives at
 *     base + ((b*H + y)*W + x)*ld + c with ld >= C (ld > C when the tensor is a
 *     channel slice of a concat buffer).  dtype is DYK_BF16 (raw uint16), DYK_F16 (raw IEEE half;
 *     forward / inference kernels only) or DYK_F32.
 *     Channel counts, ld and channel offsets must be multiples of 8 (bf16, f16) / 4 (f32)
 *     so that every pixel row starts 16-byte aligned.
 */
#ifndef DYK_HIP_H
#define DYK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYK_ABI_VERSION 5   /* 5: round 6, DykWgradDesc in-launch fold fields (sk_ws .. sk_cnt_n), dyk_conv_wgrad_fold_ws_bytes, second region of DYK_OP_MEMSET; 4: round 5, DykConvDesc split-K fields (sk_ws .. splitk), dyk_build_sha; 3: round 4, DykStemDesc fused BatchNorm-backward apply (bn_* fields); 2: round-3 descriptor layouts */

enum {
    DYK_OK = 0,
    DYK_ERR_ARG = -1,      /* invalid argument / unsupported shape */
    DYK_ERR_HIP = -2,      /* a HIP runtime call or kernel launch failed */
    DYK_ERR_UNSUPPORTED = -3,
    DYK_ERR_STATE = -4     /* plan used before bind, etc. */
};

enum { DYK_F32 = 0, DYK_BF16 = 1, DYK_U8 = 2 /* image input of dyk_image_prep only */,
       DYK_F16 = 3 /* IEEE half, inference: forward kernels only (backward, weight-gradient and BatchNorm-statistics forms
                      return DYK_ERR_UNSUPPORTED); every store saturates to +-65504, round to nearest even, NaN kept */ };

/* activation codes; the strings are the cfg `activation=` values (models.py:51-64) */
enum {
    DYK_ACT_LINEAR = 0,
    DYK_ACT_LEAKY = 1,     /* nn.LeakyReLU(0.1) */
    DYK_ACT_MISH = 2,      /* nn.Mish */
    DYK_ACT_RELU = 3,
    DYK_ACT_RELU6 = 4,
    DYK_ACT_HSIGMOID = 5,  /* nn.Hardsigmoid */
    DYK_ACT_HSWISH = 6     /* nn.Hardswish */
};

int dyk_abi_version(void);
/* digest (16 hex digits) of the kernel sources, this header and the Makefile the library was built from
 * (double-yolo-kaist_amd/dyk/buildinfo.py); the Python loader refuses a library whose digest differs from the tree's */
const char* dyk_build_sha(void);
const char* dyk_error_string(int code);

/* ------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the matrix cores (MFMA), forward and data-gradient.
 * Replaces nn.Conv2d forward (models.py:34-42, layers.py:181-182,223-231) and, with a
 * transposed weight pack and the tap table of the gradient, torch autograd's
 * conv backward-data.  One launch computes, for every position (b, yo, xo) of a launch
 * grid [B, Hg, Wg] and every output channel co:
 *     acc = sum_t sum_ci  x[b, yo*isy + tdy[t], xo*isx + tdx[t], ci] * w[twt[t]][co][ci]
 * (taps falling outside [0,Hi)x[0,Wi) contribute zero) and stores epilogue(acc) at
 *     y[b, yo*osy + ooy, xo*osx + oox, co].
 * A stride-1/2 forward conv uses (isy,isx)=stride, (osy,osx)=1; the data gradient of a
 * stride-s conv is s*s launches, one per output parity class, with (osy,osx)=s.
 * ---------------------------------------------------------------------------------- */
#define DYK_MAX_TAPS 25

enum {
    DYK_EPI_AFFINE = 1,   /* v = acc*scale[co] + shift[co]  (scale==NULL -> 1, shift==NULL -> 0) */
    DYK_EPI_RESIDUAL = 2, /* v += res[b, y, x, co]   (after the activation) */
    DYK_EPI_STATS = 4,    /* atomically add sum(acc), sum(acc^2) per channel into one of `stats_slots` replicas of
                             stats[0..Cout) / stats[Cout..2Cout): replica (workgroup id % stats_slots), 2*Cout doubles each
                             (replication bounds the atomic contention per address; dyk_bn_finalize sums the replicas) */
    DYK_EPI_ACCUM = 8,    /* y = y_old + v (gradient accumulation) */
    DYK_EPI_OUT_F32 = 16, /* y is float regardless of dtype */
    DYK_EPI_BNBWD = 32,   /* data-gradient launches only: the tensor being produced is the gradient wrt the output z of a
                             train-mode BatchNorm + activation whose raw conv output is `res` (same shape as y).  The
                             epilogue stores  da = v * act'(res*scale + shift)  instead of v and adds sum(da),
                             sum(da * (res - aux0) * aux1) per channel into a `stats` replica -- the reduce pass of that
                             BatchNorm's backward, fused (`act` = its activation; scale/shift/aux0/aux1 = its
                             scale, shift, saved mean, saved rstd).  Excludes AFFINE, RESIDUAL, STATS, ACCUM, OUT_F32. */
    DYK_EPI_BNFWD = 128,  /* with DYK_EPI_STATS, forward launches of a train-mode Conv2d + BatchNorm2d + activation block
                             (models.py:34-62) whose workgroups are ALL resident at once: conv, batch statistics, finalize and
                             normalise + activation in ONE launch.  Every workgroup stores its raw tile to y and adds its sums
                             to the statistics replicas, then arrives at the device-wide counter `bn_counter` (zero on entry;
                             the workgroup that leaves last zeroes it again, so successive launches share it without
                             re-arming) and waits until all gridDim.x workgroups have; it folds the replicas
                             of its own channels (same order and arithmetic as dyk_bn_finalize_act_fwd: scale = gamma * rstd,
                             shift = beta - mean * scale), normalises the tile it still holds in its accumulators -- rounded
                             to dtype first, i.e. exactly the values a separate pass would read back from y -- applies
                             `act` (and the RESIDUAL, if flagged) and stores it to y2 (pixel stride ldy2).  The workgroups of
                             the first pixel tile publish scale / shift / saved mean / saved rstd and update the running
                             statistics.  bf16 only; launches larger than dyk_conv_bnfwd_max_grid() are refused
                             (DYK_ERR_UNSUPPORTED): the caller may run at most TWO such launches concurrently.  A wait that
                             does not complete within 50 ms sets bit 0 of bn_counter[1] and abandons the normalise step
                             instead of hanging. */
    DYK_EPI_ADDEND = 64   /* with DYK_EPI_BNBWD only: dz = v + add[b, y, x, co] (`add`: the gradient arriving over a plain
                             [shortcut], same geometry and pixel stride as y).  The epilogue stores dz ITSELF (the next
                             link of the residual chain needs it), rounded to dtype, and reduces the sums of
                             da = dz * act'(...) computed from the rounded value; the BatchNorm-backward apply pass
                             then applies act' itself.  Removes the gradient copy of the [shortcut] and the separate
                             reduce pass for residual blocks.  add == NULL: no addend (dz = v) -- the keep-dz form alone,
                             for the LAST [shortcut] of a residual chain, whose gradient the skip branch still needs. */
};

typedef struct DykConvDesc {
    const void* x;        /* input activations, dtype */
    const void* w;        /* packed weights [ntaps_total][Cout][Cin], dtype (dyk_pack_conv_weight) */
    void* y;              /* output */
    const float* scale;   /* [Cout] or NULL */
    const float* shift;   /* [Cout] or NULL */
    const void* res;      /* residual, dtype, or NULL */
    double* stats;        /* [2*Cout] or NULL */
    const float* aux0;    /* DYK_EPI_BNBWD: saved mean [Cout] */
    const float* aux1;    /* DYK_EPI_BNBWD: saved rstd [Cout] */
    const void* add;      /* DYK_EPI_ADDEND: gradient addend, dtype, laid out like y */
    /* DYK_EPI_BNFWD (else ignored): */
    void* y2;             /* normalised + activated output, dtype */
    const float* bn_gamma;      /* [Cout] or NULL (1) */
    const float* bn_beta;       /* [Cout] or NULL (0) */
    float* bn_running_mean;     /* [Cout] or NULL: updated with bn_momentum (unbiased variance), as nn.BatchNorm2d does */
    float* bn_running_var;
    float* bn_save_mean;        /* [Cout] or NULL: batch mean / rstd for the backward pass; scale / shift above are OUTPUTS here */
    float* bn_save_rstd;
    uint32_t* bn_counter;       /* [4]: arrivals, error word, departures, unused; zero before the first launch */
    int32_t dtype;
    int32_t ldx, ldy, ldr;          /* pixel strides in elements */
    int32_t B, Hi, Wi, Cin, Cout;
    int32_t Hg, Wg;                 /* launch grid */
    int32_t Ho, Wo;                 /* full output extent */
    int32_t isy, isx, osy, osx, ooy, oox;
    int32_t ntaps;
    int8_t tdy[DYK_MAX_TAPS];
    int8_t tdx[DYK_MAX_TAPS];
    int8_t twt[DYK_MAX_TAPS];
    int8_t _pad;
    /* Output-parity classes in ONE launch (data gradient of a stride-s conv): ncls > 1 splits the tap table into
     * ncls runs, class c = taps [cls_first[c], +cls_ntaps[c]) written at output offset (cls_ooy[c], cls_oox[c]);
     * ntaps is the total, ooy/oox are ignored, every class walks the same Hg x Wg grid.  Workgroups of the classes of
     * one pixel tile get consecutive ids (one XCD): the gradient tile is fetched once and the interleaved output
     * lines meet in that L2.  ncls <= 1: a single class (ntaps, ooy, oox). */
    int8_t ncls;
    int8_t cls_first[4], cls_ntaps[4], cls_ooy[4], cls_oox[4];
    int8_t _pad2[3];
    int32_t act;                    /* DYK_ACT_* applied after the affine */
    int32_t flags;                  /* DYK_EPI_* */
    int32_t stats_slots;            /* number of stats replicas (>= 1; 0 is read as 1) */
    int32_t ldy2;                   /* DYK_EPI_BNFWD: pixel stride of y2 in elements */
    int32_t bn_count;               /* DYK_EPI_BNFWD: values per channel (B * Ho * Wo) */
    float bn_momentum, bn_eps;      /* DYK_EPI_BNFWD */
    int32_t tune;                   /* 0 = built-in heuristic; else tile configuration chosen by the plan compiler's
                                       per-shape measurement: bits 0..7 K-step bytes (64|128), 8..11 LDS ring stages
                                       (2|3|4|6), 12..15 pixel tile (0 = 128, 1 = 80, 2 = 160, 3 / 4 = halo kernel, 5 = large-tile kernels,
                                       6 = resident-weight 3x3 data gradient into 32-channel tensors; bf16, 7 = pointwise kernels),
                                       24..27 channel tile (0 = by Cout, 1 = 32, 2 = 64, 3 = 128); bits 16..23 analysis switches;
                                       1 << 28 = two K-groups per workgroup (512 threads, halves of Cin, 128-byte K step /
                                       80|160-pixel tiles).  Summary only: bits 8..11 and 24..27 mean other things under tiles 5
                                       and 7 -- the layout, field by field, is the comment at the top of csrc/conv_tune.h */
    const struct DykConvDesc* twin; /* HOST pointer or NULL.  Two-problem launch: a second problem of IDENTICAL geometry, flags and
                                       tile configuration (every non-pointer field equal) whose pointer fields x, w, y, scale,
                                       shift, res, stats, aux0, aux1, add are used -- one launch covers both, the workgroups of
                                       the second problem follow those of the first.  For the shape-identical RGB / LWIR twin
                                       backbones of a dual-stream net (models.py:288,299-303): half the launches, twice the
                                       workgroups per launch on the deep stages.  The twin's own `twin` field is ignored. */
    /* Split-K ACROSS workgroups (ABI 4).  The deep stages of the network (32x40 / 16x20 maps: 20 480 / 5 120 pixels at batch
     * 16) have 64..256 output tiles of a K loop 1 000..18 000 long: tiles large enough to feed the matrix cores leave most
     * CUs idle.  splitk = S >= 2 launches S workgroups per output tile, slice s walking the s-th share of the input-channel
     * chunks; every slice parks its fp32 accumulators in its slab of `sk_ws` (write-through stores), takes a ticket on
     * sk_cnt[tile], and the workgroup that draws the LAST ticket adds the S slabs in slice order -- the sum does not depend on
     * which slice arrives last: bit-reproducible -- and runs the epilogue of `flags` on the folded tile (statistics,
     * BatchNorm-backward reduce, ... unchanged).  No spinning: nothing depends on residency or dispatch order.
     * sk_ws: 16-byte aligned scratch private to this descriptor, sk_ws_bytes >= dyk_conv_splitk_ws_bytes(desc);
     * sk_cnt: sk_cnt_n >= number of output tiles 32-bit words, ZERO before the first launch (the last arriver re-arms its
     * word).  splitk <= 1: off.  Not combinable with twin, ncls > 1 or DYK_EPI_BNFWD; generic tiles (incl. K-grouped) and
     * the large-tile kernels carry it, the halo / resident-weight kernels fall back to their generic tile. */
    void* sk_ws;
    uint32_t* sk_cnt;
    int64_t sk_ws_bytes;
    int32_t sk_cnt_n;
    int32_t splitk;
} DykConvDesc;

int dyk_conv_igemm(const DykConvDesc* desc, void* stream);
/* largest launch (workgroups) DYK_EPI_BNFWD accepts, and the workgroups the launch of `desc` (with its tune word) would take */
int dyk_conv_bnfwd_max_grid(void);
int dyk_conv_grid(const DykConvDesc* desc);
/* split-K scratch of `desc` (its tune word and splitk): bytes of sk_ws, and (via *tiles, may be NULL) the words of sk_cnt;
 * upper bounds that hold for every kernel the tune word can select.  0 when splitk <= 1; negative error code on bad input */
int64_t dyk_conv_splitk_ws_bytes(const DykConvDesc* desc, int32_t* tiles);
/* host-only: the kernel family dyk_conv_igemm tries first for `desc` (its tune word, dtype, flags) -- the pixel-tile codes of
 * DykConvDesc.tune, 0 / 1 / 2 = generic 128- / 80- / 160-pixel tiles, 3 / 4 halo, 5 large-tile, 6 resident-weight data gradient,
 * 7 pointwise; 8 = K-grouped -- and (via *fallback_tile, may be NULL) the generic tile code that takes the problem when the
 * family refuses it, -1 = none.  Negative: error code (a word no kernel runs).  Layout and aliasing: csrc/conv_tune.h */
int dyk_conv_route(const DykConvDesc* desc, int32_t* fallback_tile);

/* ------------------------------------------------------------------------------------
 * Convolution weight gradient (split-K MFMA GEMM over output pixels, fp32 atomics):
 *     dw[twt[t]][co][ci] += sum_{b,yo,xo} dy[b,yo,xo,co] * x[b, yo*isy + tdy[t], xo*isx + tdx[t], ci]
 * dw is the fp32 gradient in the packed [tap][Cout][Cin] order (the order the master weights
 * are stored in); it is ACCUMULATED into, so the caller zeroes it when a fresh
 * gradient is wanted.  Replaces autograd's convolution_backward(weight) for models.py:34-42.
 * Rows of x / dy must be readable up to round_up(C, 16 bytes) (ld >= that).
 * ---------------------------------------------------------------------------------- */
/* one problem of a GROUPED weight-gradient launch (DykWgradDesc.group): identical geometry, own tensors */
typedef struct DykWgradGroupEntry {
    const void* x;
    const void* dy;
    float* dw;
    float* part;
} DykWgradGroupEntry;

typedef struct DykWgradDesc {
    const void* x;
    const void* dy;
    float* dw;
    float* part;                    /* NULL: partial tiles are added to dw with fp32 atomics.  Else: K split s stores its
                                       tiles (plain stores, same [tap][Cout][Cin] layout as dw) into the plane
                                       part + s * part_stride; dyk_grad_reduce later adds the planes to dw --
                                       no atomics, bit-reproducible.  Needs the split count of dyk_conv_wgrad_splits. */
    int64_t part_stride;            /* floats between the planes of consecutive splits */
    int32_t dtype;
    int32_t ldx, lddy;
    int32_t B, Hi, Wi, Cin, Ho, Wo, Cout;
    int32_t isy, isx;
    int32_t ntaps;
    int8_t tdy[DYK_MAX_TAPS];
    int8_t tdx[DYK_MAX_TAPS];
    int8_t twt[DYK_MAX_TAPS];
    int8_t _pad;
    int32_t splits;                 /* K splits; <= 0 selects automatically */
    int32_t lddw;                   /* row stride of dw in floats; <= 0 means Cin */
    int32_t tune;                   /* 0 = default; else LDS ring stages (2 | 3) | K-groups per workgroup (1 | 2) << 8 | tile cap << 24
                                       (1 = tiles of at most 64 x 64: more tiles, fewer K splits for small GEMMs) | 1 << 28: multi-tap
                                       kernel (3x3 / pad 1, bf16: dy and the x halo tile of a row segment staged once for all nine
                                       taps; ignored where it does not apply) | 2 << 28: row-block kernel (3x3 / pad 1, bf16:
                                       K steps of 128 pixels -- 256 with K-groups field = 2 -- shaped nimg x rows x columns to
                                       fit the map, 64 x 32 x 9-tap tiles; ignored where it does not apply) | 1 << 20: the caller vouches
                                       that nothing else adds to dw while the launch runs -- a launch with ONE K split may then
                                       read-add-write its tiles instead of issuing atomics (row-block kernel)
                                       | 3 << 28: pixel-streaming kernel (1x1 / stride 1, bf16: 8-wave workgroups, LDS-DMA ring of up
                                       to 8 stages; low byte = ring stages, bits 8..11 = 1 caps the tile at 64 x 64, bits 12..15 = 1:
                                       64-pixel stages for 64 x 64 tiles; ignored where it does not apply) */
    const struct DykWgradDesc* twin;/* HOST pointer or NULL: second problem of identical geometry / splits / tune whose x, dy, dw, part
                                       are used (two-problem launch, see DykConvDesc.twin) */
    /* In-launch fold of the K splits (ABI 5; part == NULL, splits >= 2; kernels: pixel-streaming 1x1): the S slices of an
     * output tile hand their accumulators over through private write-through slabs in sk_ws, take a ticket on sk_cnt[tile],
     * and the workgroup that draws the last ticket adds the S slabs IN SLICE ORDER (bit-reproducible) and adds the folded tile
     * to dw -- read-add-write when tune bit 20 vouches for a single writer, fp32 atomics otherwise.  No partial planes, no
     * dyk_grad_reduce entry.  sk_ws: 16-byte aligned, sk_ws_bytes >= dyk_conv_wgrad_fold_ws_bytes(desc); sk_cnt: sk_cnt_n >=
     * tiles 32-bit words, ZERO before the first launch (the last arriver re-arms its word).  NULL: off. */
    void* sk_ws;
    uint32_t* sk_cnt;
    int64_t sk_ws_bytes;
    int32_t sk_cnt_n;
    int32_t _pad2;
    /* Grouped launch (round 6; kernels: pixel-streaming 1x1, row-block 3x3): group_n >= 2 problems of THIS geometry / tune /
     * splits / part_stride in one launch -- the weight gradients of the repeated residual units of a stage, which become
     * ready one after the other and are nobody's input before the optimizer.  `group` is a DEVICE array of group_n entries
     * (x, dy, dw, part per problem; this descriptor's own x / dy / dw / part are validated like a single launch's and must equal
     * one member's, part's NULL-ness included: it selects plane mode for the whole group); the workgroups of problem p are
     * blocks [p * tiles * splits, (p + 1) * tiles * splits).  Every problem's result is what its own launch would give, bit for
     * bit.  Not combinable with twin or the in-launch fold. */
    const DykWgradGroupEntry* group;
    int32_t group_n;
    int32_t _pad3;
} DykWgradDesc;

int dyk_conv_wgrad(const DykWgradDesc* desc, void* stream);
/* Number of K splits (> 0) dyk_conv_wgrad will use for this descriptor (its `splits` and `tune` included): the
 * number of planes a `part` buffer must hold.  Negative = error code. */
int dyk_conv_wgrad_splits(const DykWgradDesc* desc);
/* Which kernel dyk_conv_wgrad runs for this descriptor (its `tune` included): 0 = per-tap split-K kernel, 1 = multi-tap
 * 3x3 kernel (row segments), 2 = row-block 3x3 kernel (conv_wgrad_rb.hip), 3 = pixel-streaming 1x1 kernel
 * (conv_wgrad_ps.hip).  A tune word that asks for a variant the problem is not eligible for falls back to 0.
 * Negative = error code. */
int dyk_conv_wgrad_variant(const DykWgradDesc* desc);
/* in-launch fold scratch of `desc` (its tune word and `splits` >= 2, taken literally): bytes of sk_ws, and (via *tiles, may be
 * NULL) the words of sk_cnt.  0 when the kernel the tune word selects has no in-launch fold or splits < 2; negative = error */
int64_t dyk_conv_wgrad_fold_ws_bytes(const DykWgradDesc* desc, int32_t* tiles);

/* G[g_off + i] += sum_s part[part_off + s * plane + i], i < n, for every entry of a device table: folds the per-split
 * planes written by dyk_conv_wgrad into the flat gradient buffer, one launch for many layers.  n is a multiple of 4;
 * chunk_begin = exclusive prefix sum of ceil(n / 1024) over the entries, total_chunks its total. */
typedef struct DykGradReduceEntry {
    int64_t g_off, part_off, plane;
    int32_t n, splits, chunk_begin, _pad;
} DykGradReduceEntry;
int dyk_grad_reduce(float* G, const float* part, const DykGradReduceEntry* table_dev, int32_t n_entries,
                    int32_t total_chunks, void* stream);

/* ------------------------------------------------------------------------------------
 * Channels-last elementwise / per-channel kernels share one descriptor; each entry point
 * documents the fields it reads.  Tensors a, b, out have `dtype`; npix = B*H*W pixels of C
 * channels with pixel strides lda/ldb/ldo.  p0..p3 are per-channel fp32 vectors, red a
 * fp64 reduction buffer.
 * ---------------------------------------------------------------------------------- */
enum {
    DYK_EW_ACCUM = 1,     /* out += result instead of out = result */
    DYK_EW_SKIP = 2       /* dyk_bn_act_bwd_apply: do nothing (the pass is done inside the consumer: DykStemDesc.bn_fused) */
};

typedef struct DykEwDesc {
    const void* a;
    const void* b;
    void* out;
    const float* p0;
    const float* p1;
    const float* p2;
    const float* p3;
    double* red;
    void* aux;                      /* op-specific extra pointer (max-pool argmax map, SE pooled vector, BN dgamma) */
    void* aux2;                     /* second op-specific pointer (BN dbeta) */
    int32_t dtype;
    int32_t npix, C;
    int32_t lda, ldb, ldo;
    int32_t act, flags;
    int32_t B, H, W, k;             /* spatial ops (pool / upsample) */
    float alpha, beta;
    int32_t slots;                  /* replicas of `red` (reductions; 0 is read as 1) */
    const struct DykEwDesc* twin;   /* HOST pointer or NULL: second problem with equal non-pointer fields (two-problem launch, see
                                       DykConvDesc.twin).  Honoured by dyk_bn_act_fwd, dyk_bn_finalize_act_fwd, dyk_bn_act_bwd_reduce,
                                       dyk_bn_act_bwd_apply and dyk_axpby; the other entry points return DYK_ERR_UNSUPPORTED for it */
} DykEwDesc;

/* BatchNorm2d, training mode (nn.BatchNorm2d at models.py:47, torch defaults eps=1e-5,
 * momentum=0.1): from the per-channel sum / sum-of-squares the conv epilogue accumulated in
 * stats[2C] over `count` pixels, produce scale = gamma*rstd, shift = beta - mean*scale, the
 * saved mean / rstd for backward, update running_mean / running_var (unbiased variance) and
 * reset stats to zero. */
typedef struct DykBnFinalizeDesc {
    double* stats;              /* [2C] in/out (zeroed on return) */
    const float* gamma;         /* [C] or NULL */
    const float* beta;          /* [C] or NULL */
    float* running_mean;        /* [C] or NULL (no update) */
    float* running_var;
    float* scale;               /* [C] out */
    float* shift;               /* [C] out */
    float* save_mean;           /* [C] out or NULL */
    float* save_rstd;           /* [C] out or NULL */
    int32_t C;
    int32_t count;
    float momentum, eps;
    int32_t slots;              /* replicas of stats written by the conv epilogue (0 is read as 1) */
    const struct DykBnFinalizeDesc* twin;   /* HOST pointer or NULL: second problem, equal C / count / momentum / eps / slots */
} DykBnFinalizeDesc;

int dyk_bn_finalize(const DykBnFinalizeDesc* desc, void* stream);
/* dyk_bn_finalize + dyk_bn_act_fwd in one launch: out = act(a * scale + shift) (+ b) with scale / shift derived from
 * the statistics replicas inside the kernel; scale, shift, save_mean, save_rstd and the running statistics are written
 * as by dyk_bn_finalize, but the replicas are left untouched (the caller re-arms them, e.g. one memset per pass). */
int dyk_bn_finalize_act_fwd(const DykBnFinalizeDesc* fin, const DykEwDesc* act_desc, void* stream);

/* eval-mode BatchNorm folded to scale/shift from the running statistics */
int dyk_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                const float* running_var, float eps, float* scale, float* shift, int32_t C,
                void* stream);

/* out = act(a*p0[c] + p1[c]) (+ b)           -- BN apply + activation (+ residual add of a
 * following [shortcut], layers.py:79).  p0/p1 NULL -> 1/0, b NULL -> no residual. */
int dyk_bn_act_fwd(const DykEwDesc* desc, void* stream);

/* backward of the above w.r.t. the raw conv output y (b):  a = dz, p0 = scale, p1 = shift,
 * p2 = mean, p3 = rstd.  reduce: red[c] += sum dact, red[C+c] += sum dact*xhat with
 * dact = dz*act'(y*scale+shift), spread over `slots` replicas of red (2C doubles each);
 * params: folds the replicas into replica 0, then dbeta += red[c], dgamma += red[C+c];
 * apply: out = scale*(dact - red[c]/npix - xhat*red[C+c]/npix).  The fused form (slots > 0) may read its sums as COLUMNS of
 * a wider set of replicas -- the joint reduction a convolution's DYK_EPI_BNBWD epilogue leaves for all the conv + BatchNorm
 * sections a [route] concatenates (reference models.py:116-124 / layers.py:40-48): desc->H = replica stride in doubles
 * (0 = 2C), desc->W = offset of sum(dact*xhat) from sum(dact) (0 = C), `red` points at this layer's first column. */
int dyk_bn_act_bwd_reduce(const DykEwDesc* desc, void* stream);
int dyk_bn_bwd_params(double* red, float* dgamma, float* dbeta, int32_t C, int32_t slots, void* stream);
int dyk_bn_act_bwd_apply(const DykEwDesc* desc, void* stream);

/* out = alpha*s0*a (+ beta*s1*b), s0 = p0 ? p0[0] : 1, s1 = p1 ? p1[0] : 1 (device scalars).
 * Covers channel-slice copy for [route] concat (layers.py:44), the plain [shortcut] add
 * (layers.py:79), the weighted fusion x*w0 + a*w1 (layers.py:66-73) and every gradient
 * accumulation (flags & DYK_EW_ACCUM). */
int dyk_axpby(const DykEwDesc* desc, void* stream);
/* red[0] += sum over pixels/channels of a*b   (gradient of a fusion weight).  With desc->out the same pass also stores
 * out = alpha*s0*a (+ out with DYK_EW_ACCUM), s0 = p0 ? p0[0] : 1 -- the scaled gradient copy of that source, exactly as
 * dyk_axpby would make it (autograd of layers.py:66-73 for one source in ONE pass over the gradient) */
int dyk_dot(const DykEwDesc* desc, void* stream);
/* WeightedFeatureFusion weights (layers.py:66): weff[i] = sigmoid(w[i]) * 2/n, and its backward
 * dw[i] += red[i] * 2/n * sigmoid'(w[i]) */
int dyk_wfuse_weights(const float* w, float* weff, int32_t n, void* stream);
int dyk_wfuse_bwd_params(const float* w, const double* red, float* dw, int32_t n, void* stream);

/* nn.Upsample(scale_factor=2) nearest (models.py:100-101): a [B,H,W,C] -> out [B,2H,2W,C];
 * backward: a = dout [B,2H,2W,C] -> out = din [B,H,W,C] (sum of the 2x2 block). */
int dyk_upsample2x_fwd(const DykEwDesc* desc, void* stream);
int dyk_upsample2x_bwd(const DykEwDesc* desc, void* stream);

/* nn.MaxPool2d(k, stride, padding=(k-1)//2) (models.py:91-94), k <= 15; the stride travels in `slots` (0 / 1 = stride 1,
 * the SPP pools of the shipped cfgs).  H, W are the INPUT extents; the output is [(H+2p-k)/stride+1, (W+2p-k)/stride+1].
 * argmax is a uint8 [B*Ho*Wo][C] map of the window position (dy*k+dx) of the first maximum in scan order
 * (torch CPU tie rule); backward (a = dout, out = din) gathers dout through it (deterministic, no atomics). */
int dyk_maxpool_fwd(const DykEwDesc* desc, uint8_t* argmax, void* stream);
int dyk_maxpool_bwd(const DykEwDesc* desc, const uint8_t* argmax, void* stream);

/* SqueezeExcitation (layers.py:175-190).
 *   dyk_se_pool : pooled[b][c] = alpha * sum_hw a[b,hw,c] * (b ? b[b,hw,c] : 1)
 *                 (alpha = 1/HW gives adaptive_avg_pool2d; with b = dz it is the gradient of the
 *                 per-channel scale).  desc->aux2 (optional): scratch of DYK_SE_POOL_SPLITS * B * C floats;
 *                 with it the pixels of an image are reduced by up to DYK_SE_POOL_SPLITS workgroups whose
 *                 partial sums are folded in a fixed order (same result from run to run)
 *   dyk_se_fc_fwd : scale = hardsigmoid(W2 relu(W1 pooled + b1) + b2); two launches that spread the rows of W1 / W2 over
 *                   the chip.  Needs `ws` (B*(C + 2*Cs) floats): h = relu(..) and t2 = W2 h + b2 are parked there
 *   dyk_se_scale  : out[b,hw,c] = a[b,hw,c]*p0[b*C+c] (+ alpha*p1[b*C+c])
 *                   With desc->red set (backward of a block whose input is the activated output of a conv + BatchNorm layer,
 *                   autograd of models.py:47-56 behind layers.py:188): b = that layer's raw conv output, p2 = its
 *                   scale | shift | mean | rstd vectors [4][C], act = its activation; sum(da), sum(da * xhat) with
 *                   da = out * act'(scale * b + shift) go to the `slots` fp64 replicas red[slots][2][C] exactly as
 *                   dyk_bn_act_bwd_reduce over `out` would leave them; `out` itself stays the gradient
 *   dyk_se_fc_bwd : from dscale = d(loss)/d(scale) produce dpooled and accumulate dW1,db1,dW2,db2.  MUST follow
 *                   dyk_se_fc_fwd on the same `ws` (it reads the h and t2 the forward call parked; nothing is
 *                   recomputed).  Three launches: dt1 = relu'(h) * W2^T (dscale * hardsigmoid'(t2)) -> ws,
 *                   dpooled = W1^T dt1, then one thread per weight element sums its outer products over the
 *                   batch -- no atomics on the weight gradients, every sum in a fixed order.
 *                   dyk_se_fc_bwd may be called in two halves: with dw1 = db1 = dw2 = db2 = NULL it computes dpooled
 *                   (and dt1 into ws) only; with dpooled = NULL only the parameter gradients, from what the first
 *                   half left in ws -- the parameter half is not on the path to dx (dyk/plan.py issues it as its own
 *                   command so that the dependency scheduler can move it off the backward chain). */
typedef struct DykSeFcDesc {
    const float* pooled;   /* [B][C] */
    const float* w1;       /* [Cs][C]  fc1.weight */
    const float* b1;       /* [Cs] */
    const float* w2;       /* [C][Cs]  fc2.weight */
    const float* b2;       /* [C] */
    float* scale;          /* [B][C] out (fwd) */
    const float* dscale;   /* [B][C] (bwd) */
    float* dpooled;        /* [B][C] out (bwd) */
    float* dw1; float* db1; float* dw2; float* db2;   /* accumulated (bwd) */
    float* ws;             /* B*(C + 2*Cs) floats: h [B][Cs] (fwd) | dt1 [B][Cs] (bwd) | t2 [B][C] (fwd) */
    int32_t B, C, Cs;
} DykSeFcDesc;
#define DYK_SE_POOL_SPLITS 16
int dyk_se_pool(const DykEwDesc* desc, float* pooled, void* stream);
int dyk_se_fc_fwd(const DykSeFcDesc* desc, void* stream);
int dyk_se_fc_bwd(const DykSeFcDesc* desc, void* stream);
int dyk_se_scale(const DykEwDesc* desc, void* stream);

/* YOLOLayer training-mode reshape (models.py:229): head conv output y [B,ny,nx,ld] fp32 with
 * channel = a*no + o  ->  p [B,na,ny,nx,no] fp32.  Backward scatters dp back into a zero-padded
 * dy [B,ny,nx,ld] of `dtype` and, if dbias != NULL, accumulates the head bias gradient. */
int dyk_head_permute_fwd(const float* y, float* p, int32_t B, int32_t ny, int32_t nx, int32_t na,
                         int32_t no, int32_t ld, void* stream);
int dyk_head_permute_bwd(const float* dp, void* dy, float* dbias, int32_t B, int32_t ny, int32_t nx,
                         int32_t na, int32_t no, int32_t ld, int32_t dtype, void* stream);

/* Input path of the harness (train_utils/kaist_train_eval_utils.py:54-55 `imgs.to(device).float() / 255.0`, and under
 * multi-scale training :59-71 `F.interpolate(imgs, size=ns, mode='bilinear', align_corners=False)`) as one pass:
 * src [planes = B*C][Hi][Wi] of src_dtype (DYK_U8 loader output, kaist_dataset.py:385-386, or DYK_F32)
 *   -> dst f32 [planes][Ho][Wo] = bilinear(src / div).  Hi == Ho && Wi == Wo is the plain conversion.
 * Source index / lambda arithmetic is ATen's (scale = in/out, src = scale*(dst+0.5)-0.5 clamped at 0). */
int dyk_image_prep(const void* src, float* dst, int32_t planes, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                   int32_t src_dtype, float div, void* stream);

/* First-layer patch gather: torch NCHW fp32 image batch -> channels-last patches
 * out[b,yo,xo,(kh*k+kw)*Cin + c] = in[b,c,yo*stride+kh-pad,xo*stride+kw-pad]*mul (zero padded up
 * to ld channels), which turns the Cin=3 stem conv (models.py:35-36) into a 1x1 MFMA conv. */
int dyk_patch_gather(const float* in, void* out, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t k,
                     int32_t stride, int32_t pad, int32_t ld, float mul, int32_t dtype, void* stream);

/* Weight pack: torch OIHW float32 [Cout][Cin][kh][kw] (nn.Conv2d.weight, models.py:34)
 *   transposed == 0:  out[t][co][ci] = w[co][ci][t]     (forward)
 *   transposed == 1:  out[t][ci][co] = w[co][ci][t]     (data gradient: roles of Cin/Cout swap)
 * with t = kh_index*kw + kw_index; rows are padded with zeros up to Cin_pad / Cout_pad. */
int dyk_pack_conv_weight(const float* w_oihw, void* out, int32_t Cout, int32_t Cin, int32_t kh,
                         int32_t kw, int32_t Cout_pad, int32_t Cin_pad, int32_t transposed,
                         int32_t dtype, void* stream);

/* Layout/precision conversion at the drop-in boundary (YOLO.forward takes torch NCHW float32,
 * models.py:279): out[b,y,x,c] = in[b,c,y,x] * mul for c < C, zero for C <= c < Cpad. */
int dyk_nchw_to_nhwc(const float* in, void* out, int32_t B, int32_t C, int32_t H, int32_t W,
                     int32_t Cpad, int32_t ldo, float mul, int32_t dtype, void* stream);
int dyk_nhwc_to_nchw(const void* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                     int32_t ldi, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Depthwise convolution (nn.Conv2d(groups=C), reference models.py:41 for `groups=` sections and
 * layers.py:223-224 for DepthwiseSeparableConv2d), square kernel k <= 7, zero padding `pad`, any stride >= 1 (stride 1 and 2
 * at k 3 / 5 have kernels of their own, everything else runs on the generic ones).
 * w is the fp32 master weight in tap-major order [k*k][C] (the parameter store layout).
 *   dyk_dwconv_fwd   : y[b,yo,xo,c] = sum_t x[b, yo*s+kh-pad, xo*s+kw-pad, c] * w[t][c]
 *                      stats (optional): replicated fp64 [slots][2][C] sum / sum of squares of y
 *   dyk_dwconv_dgrad : x := gradient wrt the conv input [B,Hi,Wi,C] (written, or accumulated with
 *                      DYK_EW_ACCUM), y := gradient wrt the conv output [B,Ho,Wo,C] (read)
 *   dyk_dwconv_wgrad : dw[t][c] += sum_p y[p][c] * x[src(p,t)][c]     (y = output gradient)
 * In the two gradient entry points the roles follow the tensor, not the data direction:
 * x/ldx/Hi/Wi always describe the conv-input-shaped tensor, y/ldy/Ho/Wo the conv-output-shaped one.
 * ---------------------------------------------------------------------------------- */
typedef struct DykDwDesc {
    void* x;
    void* y;
    const float* w;
    float* dw;
    double* stats;
    float* part;                    /* dyk_dwconv_wgrad only.  NULL: workgroups add their sums to dw with fp32 atomics.  Else
                                       workgroup row r (of dyk_dwconv_wgrad_rows) stores them into the plane
                                       part + r * k*k*C; dyk_grad_reduce folds the planes (reproducible). */
    int32_t dtype, ldx, ldy;
    int32_t B, Hi, Wi, Ho, Wo, C;
    int32_t k, stride, pad;
    int32_t flags, stats_slots;
    /* dyk_dwconv_dgrad only, res != NULL: the BatchNorm-backward reduce of the layer that produced the conv input is
     * folded into this data gradient (as DYK_EPI_BNBWD does for dyk_conv_igemm): with u = res (the producer's raw conv
     * output, row length ldr), da = dx * act'(scale*u + shift) is stored instead of dx and sum(da), sum(da * (u-mean)*rstd)
     * are added to the fp64 replicas stats[stats_slots][2][C].  bn = scale | shift | mean | rstd, C floats each.
     * Stride 1, k in {3, 5}, bf16, no DYK_EW_ACCUM. */
    const void* res;
    const float* bn;
    int32_t ldr, act;
    /* dyk_dwconv_fwd / dyk_dwconv_wgrad, pre != NULL (round 5): x is the RAW output u of a train-mode Conv2d + BatchNorm2d +
     * activation block (the 1x1 expansion conv of a MobileNet block, reference models.py:34-62 in front of :41 groups=C) whose
     * normalise + activation pass was NOT run: the kernel forms z = dtype(act(scale * u + shift)) on load -- exactly the
     * values that pass would have stored -- and convolves / correlates z.  pre = scale | shift, C floats each (the first half
     * of the `bn` layout), pre_act = that block's DYK_ACT_*.  Padding taps stay zero (the affine is not applied outside the
     * image).  Forward: the LDS-tiled stride-1 kernel only (dyk_dwconv_tile_ok), else DYK_ERR_UNSUPPORTED. */
    const float* pre;
    int32_t pre_act, _pad;
} DykDwDesc;
int dyk_dwconv_fwd(const DykDwDesc* desc, void* stream);
/* 1 when dyk_dwconv_fwd runs a descriptor of this shape on the LDS-tiled kernel (stride 1, k in {3, 5}, bf16 or fp16, tile fits;
 * `w`, `stats` and `pre` are not looked at): the precondition of `pre` in the forward and, in bf16, of `res` in the data gradient;
 * 0 otherwise; negative = error code */
int dyk_dwconv_tile_ok(const DykDwDesc* desc);
int dyk_dwconv_dgrad(const DykDwDesc* desc, void* stream);
int dyk_dwconv_wgrad(const DykDwDesc* desc, void* stream);
/* number of workgroup rows (= planes of `part`) dyk_dwconv_wgrad uses for this descriptor; negative = error code.  Stride-1
 * 3x3 / 5x5 bf16 problems run on the LDS-tiled persistent kernel (round 5: one pass over dy and x, the next tile's loads in flight
 * while a tile is computed; planes = its workgroups per channel group), everything else on the row kernel (planes = workgroup rows
 * per kernel row); the count depends on the descriptor's shape fields only, never on `part` / `dw`. */
int dyk_dwconv_wgrad_rows(const DykDwDesc* desc);

/* ------------------------------------------------------------------------------------
 * Parameter staging.  Master parameters and gradients are fp32, conv weights stored
 * tap-major [kh*kw][Cout][Cin] (DESIGN.md "parameter store").
 *   dyk_cast_f32       : dst[i] = (dtype) src[i]                      (whole flat buffer, one launch)
 *   dyk_cast_pad_rows  : dst[r][c] = src[r][c] (c < C), 0 (C <= c < Cpad)   (stem weights, K padded)
 *   dyk_transpose_taps : for each entry e of a device table: dst_e[t][ci][co] = src_e[t][co][ci]
 *                        (weights for the data-gradient GEMM), one launch for all layers; dst rows may be
 *                        padded to dst_ld (channel counts that are not a multiple of the GEMM K step).
 * ---------------------------------------------------------------------------------- */
typedef struct DykTransposeEntry {
    int64_t src_off;      /* element offset into src (fp32) */
    int64_t dst_off;      /* element offset into dst (dtype) */
    int32_t taps, rows, cols;   /* src is [taps][rows][cols] */
    int32_t tile_begin;   /* first 32x32 tile index of this entry (exclusive prefix sum) */
    int32_t dst_ld;       /* row length of dst (>= rows, <= rows rounded up to 32; 0 = rows); the tail is zero-filled */
    int32_t _pad;
} DykTransposeEntry;
/* dyk_cast_pad_table: every K-padded weight pack of a model in ONE launch (the MobileNet cfgs have 68 of them: 68 launches of
 * 3 us on the caller's stream at every step boundary, round 5).  Entry e: dst_e[r][c] = (dtype) src_e[r][c] for c < cols,
 * 0 for cols <= c < cpad; with transpose_f32 set dst_e is fp32 [cols][rows] = the transpose of src_e (no padding).  blk_begin =
 * exclusive prefix sum of ceil(elements_e / 2048) over the entries; total_blocks = its end. */
typedef struct DykPadEntry {
    const float* src;
    void* dst;
    int32_t rows, cols, cpad;
    int32_t blk_begin;
    int32_t transpose_f32;
    int32_t _pad;
} DykPadEntry;
int dyk_cast_pad_table(const DykPadEntry* table_dev, int32_t n_entries, int32_t total_blocks, int32_t dtype, void* stream);
int dyk_cast_f32(const float* src, void* dst, int64_t n, int32_t dtype, void* stream);
int dyk_cast_pad_rows(const float* src, void* dst, int32_t R, int32_t C, int32_t Cpad, int32_t dtype, void* stream);
int dyk_transpose_taps(const float* src, void* dst, const DykTransposeEntry* table_dev, int32_t n_entries,
                       int32_t total_tiles, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Command lists.  A compiled plan (one per cfg x batch shape x dtype x mode) is a flat array of
 * commands whose descriptors already hold resolved device pointers; dyk_run_commands enqueues
 * them in order on `stream` from native code (no per-kernel Python / ctypes overhead).
 * desc points at the struct named next to each op code; DykMiscDesc carries the arguments of the
 * entry points that take scalars (slot assignment listed per op).
 * ---------------------------------------------------------------------------------- */
typedef struct DykMiscDesc {
    void* p[6];
    int64_t n;
    int32_t i[12];
    float f[4];
} DykMiscDesc;

enum {
    DYK_OP_CONV = 1,            /* DykConvDesc        -> dyk_conv_igemm */
    DYK_OP_WGRAD = 2,           /* DykWgradDesc       -> dyk_conv_wgrad */
    DYK_OP_BN_FINALIZE = 3,     /* DykBnFinalizeDesc  -> dyk_bn_finalize */
    DYK_OP_BN_ACT_FWD = 4,      /* DykEwDesc */
    DYK_OP_BN_BWD_REDUCE = 5,   /* DykEwDesc */
    DYK_OP_BN_BWD_APPLY = 6,    /* DykEwDesc */
    DYK_OP_AXPBY = 7,           /* DykEwDesc */
    DYK_OP_DOT = 8,             /* DykEwDesc */
    DYK_OP_UPSAMPLE_FWD = 9,    /* DykEwDesc */
    DYK_OP_UPSAMPLE_BWD = 10,   /* DykEwDesc */
    DYK_OP_MAXPOOL_FWD = 11,    /* DykEwDesc, aux = argmax */
    DYK_OP_MAXPOOL_BWD = 12,    /* DykEwDesc, aux = argmax */
    DYK_OP_SE_POOL = 13,        /* DykEwDesc, aux = pooled */
    DYK_OP_SE_FC_FWD = 14,      /* DykSeFcDesc */
    DYK_OP_SE_FC_BWD = 15,      /* DykSeFcDesc */
    DYK_OP_SE_SCALE = 16,       /* DykEwDesc */
    DYK_OP_BN_BWD_PARAMS = 17,  /* Misc: p0=red p1=dgamma p2=dbeta i0=C i1=slots */
    DYK_OP_BN_FOLD = 18,        /* Misc: p0=gamma p1=beta p2=rmean p3=rvar p4=scale p5=shift i0=C f0=eps */
    DYK_OP_WFUSE_WEIGHTS = 19,  /* Misc: p0=w p1=weff i0=n */
    DYK_OP_WFUSE_BWD_PARAMS = 20, /* Misc: p0=w p1=red p2=dw i0=n */
    DYK_OP_HEAD_PERMUTE_FWD = 21, /* Misc: p0=y p1=p i0=B i1=ny i2=nx i3=na i4=no i5=ld */
    DYK_OP_HEAD_PERMUTE_BWD = 22, /* Misc: p0=dp p1=dy p2=dbias i0..i5 as fwd, i6=dtype */
    DYK_OP_PATCH_GATHER = 23,   /* Misc: p0=in p1=out i0=B i1=Cin i2=H i3=W i4=k i5=stride i6=pad i7=ld i8=dtype f0=mul */
    DYK_OP_MEMSET = 24,         /* Misc: p0=ptr n=bytes i0=value; optional second region p1=ptr i1=bytes (zeros) */
    DYK_OP_YOLO_DECODE = 25,    /* DykDecodeDesc */
    DYK_OP_DW_FWD = 26,         /* DykDwDesc -> dyk_dwconv_fwd */
    DYK_OP_DW_DGRAD = 27,       /* DykDwDesc -> dyk_dwconv_dgrad */
    DYK_OP_DW_WGRAD = 28,       /* DykDwDesc -> dyk_dwconv_wgrad */
    DYK_OP_CAST_PAD_ROWS = 29,  /* Misc: p0=src p1=dst i0=R i1=C i2=Cpad i3=dtype */
    DYK_OP_BN_FWD_FUSED = 30,   /* Misc: p0=DykBnFinalizeDesc* p1=DykEwDesc* -> dyk_bn_finalize_act_fwd */
    DYK_OP_GRAD_REDUCE = 31,    /* Misc: p0=G p1=part p2=table i0=n_entries i1=total_chunks -> dyk_grad_reduce */
    DYK_OP_STEM_FWD = 32,       /* DykStemDesc -> dyk_stem_conv_fwd */
    DYK_OP_STEM_WGRAD = 33,     /* DykStemDesc -> dyk_stem_conv_wgrad */
    DYK_OP_HEAD_DECODE = 34,    /* DykHeadDecodeDesc -> dyk_head_decode */
    DYK_OP_COUNT_
};

typedef struct DykCommand {
    int32_t op;
    int32_t lane;         /* scheduling hints for dyk_run_commands_overlap (ignored by dyk_run_commands):
                             bit 0 = belongs to the second, independent branch (the LWIR backbone of a dual-stream
                             net); bit 1 = fork point (the branch may start once everything before this command is
                             done); bit 2 = join (this command needs both branches); bit 3 = a weight-gradient command that
                             stays on its own stream (the tail of a backward list: balances the side stream) */
    const void* desc;
} DykCommand;

/* One two-problem launch of commands a and b (same op, descriptors equal in every non-pointer field; see DykConvDesc.twin).
 * Ops: DYK_OP_CONV, DYK_OP_WGRAD, DYK_OP_BN_FINALIZE, DYK_OP_BN_ACT_FWD, DYK_OP_BN_FWD_FUSED, DYK_OP_BN_BWD_REDUCE,
 * DYK_OP_BN_BWD_APPLY, DYK_OP_AXPBY; DYK_ERR_UNSUPPORTED otherwise, DYK_ERR_ARG when the two descriptors differ in shape. */
int dyk_run_command_pair(const DykCommand* a, const DykCommand* b, void* stream);

/* Enqueue cmds[0..n) in order.  Stops at the first failure and returns its code; *failed_index
 * (may be NULL) receives the index of the failing command. */
int dyk_run_commands(const DykCommand* cmds, int32_t n, void* stream, int32_t* failed_index);
/* Same result, more concurrency: commands tagged as the second branch (DykCommand.lane) run on a library-owned
 * stream between their fork and join points, and weight-gradient commands (DYK_OP_WGRAD, DYK_OP_DW_WGRAD; nothing
 * in a backward pass reads dW) on another one, each behind an event that covers everything enqueued before it on
 * the issuing stream.  `stream` waits for both side streams before the call returns (no host synchronisation). */
int dyk_run_commands_overlap(const DykCommand* cmds, int32_t n, void* stream, int32_t* failed_index);

/* ------------------------------------------------------------------------------------
 * YOLOLayer inference decode (models.py:234-258): p [B,na,ny,nx,no] fp32 raw logits ->
 * io rows [row_offset + (a*ny + y)*nx + x] of a [B, rows_total, no] fp32 buffer:
 *   v3: xy = (sigmoid(t) + grid)*stride, wh = exp(t)*anchor_vec*stride, rest = sigmoid
 *   v4: s = sigmoid(t); xy = (s*2 - 0.5 + grid)*stride, wh = (s*2)^2*anchor_vec*stride, rest = s
 * ---------------------------------------------------------------------------------- */
typedef struct DykDecodeDesc {
    const float* p;
    float* io;
    int32_t B, na, ny, nx, no;
    int32_t rows_total, row_offset;
    int32_t v4;
    float stride;
    float anchor_vec[2 * 8];        /* (w, h) per anchor, already divided by stride (models.py:182) */
} DykDecodeDesc;
int dyk_yolo_decode(const DykDecodeDesc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * One-launch inference head for wide heads (na*no > 32): y [B,ny,nx,ld] fp32, the head conv's
 * output (channel = a*no + o, ld >= na*no), is read once and leaves BOTH
 *   p  [B,na,ny,nx,no] fp32   = what dyk_head_permute_fwd writes, and
 *   io rows [row_offset + (a*ny + y)*nx + x] of [B, rows_total, no] = what dyk_yolo_decode writes
 * from that p, bit for bit.  One thread per output element, consecutive threads on consecutive o.
 * ---------------------------------------------------------------------------------- */
typedef struct DykHeadDecodeDesc {
    const float* y;
    float* p;
    float* io;
    int32_t B, na, ny, nx, no, ld;
    int32_t rows_total, row_offset;
    int32_t v4;
    float stride;
    float anchor_vec[2 * 8];        /* as DykDecodeDesc.anchor_vec */
} DykHeadDecodeDesc;
int dyk_head_decode(const DykHeadDecodeDesc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * Target assignment and loss (build_utils/utils.py:209-384).
 * dyk_build_targets: for every head h and every (anchor a, target t) pair in anchor-major order,
 *   keep the pair iff wh_iou(anchor_vec[h][a], (w,h)*grid) > iou_t and emit
 *   indices[h][0..3][m] = (image, anchor, gj, gi) (int64, truncation, no clamping), tbox[h][m] =
 *   (gx-gi, gy-gj, gw, gh), anch[h][m], tcls[h][m]; counts[h] = number of matches.  Arrays are
 *   sized for cap = na*nt matches per head: indices [nheads][4][cap], tbox [nheads][cap][4],
 *   anch [nheads][cap][2], tcls [nheads][cap].  targets is [nt][6] = (image, class, xc, yc, w, h).
 * dyk_yolo_loss: runs the assignment, then the CIoU/GIoU box loss, the objectness BCE over all
 *   cells (targets scattered with last-match-wins) and the class BCE (nc > 1), writes
 *   out[0..2] = (box, obj, cls) * hyp gains and the gradient of each term w.r.t. the logits into
 *   dp[h] (box -> channels 0..3, obj -> 4, cls -> 5..): the three terms touch disjoint channels, so
 *   dyk_loss_scale_grads can apply the three upstream gradients afterwards.
 *   *flag gets bit 0 set if a target indexed outside the grid (the reference raises IndexError).
 * ---------------------------------------------------------------------------------- */
typedef struct DykTargetsDesc {
    const float* targets;
    int32_t nt, nheads, na;
    int32_t ny[3], nx[3];
    float anchor_vec[3][16];
    float iou_t;
    int32_t* counts;       /* [nheads] */
    int64_t* indices;
    float* tbox;
    float* anch;
    int64_t* tcls;
} DykTargetsDesc;

typedef struct DykLossDesc {
    const float* p[3];     /* [B][na][ny][nx][no] raw logits */
    float* dp[3];          /* same shape, out */
    float* tobj[3];        /* [B][na][ny][nx] scratch */
    int32_t nheads, B, no, nc;
    int32_t v4;            /* box parameterisation: 'yolov4' in cfg (utils.py:252) */
    int32_t ciou;          /* 'ciou' in hyp (utils.py:264), else GIoU */
    float hyp_box, hyp_obj, hyp_cls, cls_pw, obj_pw, gr;
    float fl_gamma;        /* hyp['fl_gamma'] > 0: both BCE terms wrapped in FocalLoss (utils.py:174-201, :236-238); 0 = plain BCE */
    float fl_alpha;        /* FocalLoss alpha (utils.py:176 default 0.25; read only when fl_gamma > 0) */
    double* acc;           /* [12] scratch */
    float* out;            /* [3] */
    int32_t* flag;         /* bit 0 is SET when a target falls outside the grid; dyk_yolo_loss clears it first, like dp / tobj /
                              acc.  Two back-to-back layouts get ONE fill for everything: acc | flag | 4 spare bytes | dp[0] |
                              dp[1] | .. | tobj[0] | ..  (acc leads: 8-byte aligned for any grid) and dp[0] | .. | tobj[..] | acc
                              | flag; any other layout takes one fill per buffer */
} DykLossDesc;

int dyk_build_targets(const DykTargetsDesc* desc, void* stream);
int dyk_yolo_loss(const DykLossDesc* desc, const DykTargetsDesc* targets, void* stream);
int dyk_loss_scale_grads(float* dp, int64_t n, int32_t no, const float* g3, void* stream);
/* The same with the three upstream gradients as separate device scalars (NULL = 0: the term is not in the differentiated sum) --
 * autograd hands them over separately (reference utils.py:287-293 returns three tensors), no concatenation launch; dp may be the
 * back-to-back gradient buffers of all heads (one launch). */
int dyk_loss_scale_grads3(float* dp, int64_t n, int32_t no, const float* gbox, const float* gobj, const float* gcls, void* stream);

/* ------------------------------------------------------------------------------------
 * non_max_suppression (build_utils/utils.py:387-464) incl. torchvision.ops.nms (:448), one
 * workgroup per image.  pred [B][N][no] decoded boxes (cx,cy,w,h,obj,cls...).  Per image b:
 *   counts[b] = k <= max_num, out[b][0..k) = (x1,y1,x2,y2,conf,cls) in descending-score order,
 *   out_rows[b][0..k) = row of pred each detection came from.
 * Semantics: strict `>` thresholds, 2 < w,h < 4096, conf = obj*cls, best class unless
 * multi_label (and nc > 1), optional class filter, per-class offset 4096 unless agnostic, greedy
 * suppression of IoU > iou_thres in stable descending score order, first max_num kept.  The
 * reference's 10 s wall-clock bail-out (:461-462) is deliberately not reproduced.
 * ws: B * ws_per_image bytes, ws_per_image >= dyk_nms_workspace_bytes(N, no, multi_label).
 *
 * dyk_nms_ex(desc, flags, stream): dyk_nms(d, s) == dyk_nms_ex(d, 0, s); unknown flag bits -> DYK_ERR_ARG.
 * DYK_NMS_MERGE: the reference's merge-NMS stage (utils.py:398 `merge`, :450-454; False as shipped), in the same
 * launch.  Per image with candidate count n (after every filter; in multi_label mode one row can give several) and
 * only when 1 < n < 3000 (:450, both strict -- otherwise the output is the plain one bit for bit):
 *   member(k, j) = box_iou(boxes[i[k]], boxes[j]) > iou_thres  (:452, box_iou :141-163: inter / (area_k + area_j -
 *                  inter) in fp32 on the class-offset boxes of :447 as rounded, strict), over ALL n candidates -- the
 *                  suppressed ones, the kept box itself and survivors cut off by max_num;
 *   out[b][k][0..4) = sum_j member * conf_j * xyxy_j / sum_j member * conf_j  (:453-454) over the un-offset corners
 *                  of the original candidates (the right-hand side never sees a merged box).
 * conf, cls, order, counts and out_rows are those of the plain call.  Each coordinate lies within
 * 2^-23 * max(|exact|, 1) of the exact weighted mean of the fp32 inputs (fp64 accumulation, one rounding to fp32;
 * the reference's torch.mm sums in fp32) and is bit-identical from run to run.  The workspace size does not change.
 * The reference's try/except around the merge and its print are not reproduced.
 * ---------------------------------------------------------------------------------- */
typedef struct DykNmsDesc {
    const float* pred;
    float* out;            /* [B][max_num][6] */
    int32_t* out_rows;     /* [B][max_num] */
    int32_t* counts;       /* [B] */
    void* ws;
    int64_t ws_per_image;
    int32_t B, N, no;
    float conf_thres, iou_thres;
    int32_t multi_label, agnostic, max_num;
    int32_t n_classes;     /* 0 = no class filter */
    int32_t classes[16];
} DykNmsDesc;
int64_t dyk_nms_workspace_bytes(int32_t N, int32_t no, int32_t multi_label);
int dyk_nms(const DykNmsDesc* desc, void* stream);
#define DYK_NMS_MERGE 1
int dyk_nms_ex(const DykNmsDesc* desc, int32_t flags, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-label non_max_suppression with a bounded workspace (the `multi_label` branch of build_utils/utils.py:422-424,
 * `(x[:, 5:] > conf_thres).nonzero()`, in front of the same :430-431, :446-454 as above).  dyk_nms_ex with
 * multi_label = 1 sizes its workspace for N * nc candidates and visits every (row, class) pair with a thread of its
 * own; dyk_nms_rows holds at most cand_cap candidates per image and walks each alive row with one wavefront, 64
 * consecutive class scores per load.  One workgroup per image.  The descriptor's leading fields are DykNmsDesc's with
 * the same meaning.  The argument checks are those of dyk_nms_ex plus cand_cap >= 1, n_cand != NULL, the workspace size,
 * and multi_label != 0 with no > 6: a best-class call has one candidate per row at most and stays with dyk_nms_ex
 * (DYK_ERR_ARG here).  Per image b:
 *   n_cand[b] = exact number of candidates (rows x classes that pass every filter), always written;
 *   n_cand[b] <= cand_cap: counts[b], out[b], out_rows[b] are bit for bit those of dyk_nms_ex(desc, flags) -- the
 *                candidates are the same set in the same (row, class) order with the same fp32 bits, and sort,
 *                suppression and merge are the same device code (csrc/nms_phases.h);
 *   n_cand[b] >  cand_cap: counts[b] = -1 and nothing else of the image is written (out, out_rows, and the workspace
 *                beyond the per-row arrays); the other images are not affected.  The caller repeats the batch through
 *                dyk_nms_ex, or with cand_cap >= max(n_cand).
 * ws: B * ws_per_image bytes, ws_per_image >= dyk_nms_rows_workspace_bytes(N, cand_cap)
 *   = dyk_nms_workspace_bytes(cand_cap, 6, 0) + roundup(8 * N, 256)
 *   = roundup(8 * P(cand_cap) + 28 * cand_cap, 256) + roundup(8 * N, 256),  P(c) the power of two >= c:
 * the sort keys and candidates of a best-class call over cand_cap rows, then rowlist[N] (alive rows, ascending) and
 * rowoff[N] (candidates per alive row, then their exclusive prefix sum).  No class count in it.
 * ---------------------------------------------------------------------------------- */
typedef struct DykNmsRowsDesc {
    const float* pred;
    float* out;            /* [B][max_num][6] */
    int32_t* out_rows;     /* [B][max_num] */
    int32_t* counts;       /* [B]; -1: the image has more than cand_cap candidates */
    void* ws;
    int64_t ws_per_image;
    int32_t B, N, no;
    float conf_thres, iou_thres;
    int32_t multi_label, agnostic, max_num;
    int32_t n_classes;     /* 0 = no class filter */
    int32_t classes[16];
    int32_t cand_cap;      /* candidates one image may hold in ws */
    int32_t* n_cand;       /* [B] out: exact candidate count of the image */
} DykNmsRowsDesc;
int64_t dyk_nms_rows_workspace_bytes(int32_t N, int32_t cand_cap);
int dyk_nms_rows(const DykNmsRowsDesc* desc, int32_t flags, void* stream);   /* flags: DYK_NMS_MERGE or 0 */

/* ------------------------------------------------------------------------------------
 * Fused optimizer step over the flat parameter store (replaces the per-tensor torch.optim.Adam /
 * optim.SGD(nesterov=True) updates of reference train.py:85-91; same update rule incl. L2
 * weight_decay added to the gradient).  n must be a multiple of 4, pointers 16-byte aligned.
 *   grad_scale : multiplies the gradient first (1/world_size after an all-reduce SUM, 1/loss_scale)
 *   wc         : if not NULL, also writes the bf16 copy of the updated parameters (same offsets)
 *   zero_grad  : if non-zero, clears g after use (next backward accumulates into zeros)
 *   mask       : if not NULL, one byte per element, 0 = frozen: no update, no decay, moments untouched (the
 *                reference builds its optimizer from `p.requires_grad` parameters only, train.py:84); a parameter's
 *                elements start at multiples of 64, so four consecutive bytes always agree
 * dyk_adam_step : m = exp_avg, v = exp_avg_sq, beta1/beta2/eps, step = 1-based step count
 * dyk_sgd_step  : m = momentum buffer, beta1 = momentum, Nesterov, dampening 0 (v, beta2, eps unused)
 * ---------------------------------------------------------------------------------- */
typedef struct DykOptimDesc {
    float* p;
    float* g;
    float* m;
    float* v;
    void* wc;
    const uint8_t* mask;
    int64_t n;
    float lr, beta1, beta2, eps, weight_decay, grad_scale;
    int32_t step;
    int32_t zero_grad;
} DykOptimDesc;
int dyk_adam_step(const DykOptimDesc* desc, void* stream);
int dyk_sgd_step(const DykOptimDesc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * Non-finite guard and gradient clipping of the fused optimizers, decided on the device (replaces what the reference
 * harness gets from amp.GradScaler -- scaler.step() skipping a step whose gradients hold inf / NaN,
 * train_utils/kaist_train_eval_utils.py:44,103-108 -- and torch.nn.utils.clip_grad_norm_ over the gradient views, without
 * the per-tensor kernels and without the host synchronisation of `found_inf.item()`).
 *
 * dyk_grad_stats : two launches on `stream` over the flat gradient buffer g[0..n):
 *   partials : grid = min(ceil(n/4 / 256), 1024) blocks of 256 threads (a function of n only).  Every live element
 *              (mask == NULL, or the 4 mask bytes of its 16-byte vector not all 0) is taken as x = fl32(g * grad_scale), the
 *              value the update consumes; !(|x| <= FLT_MAX) counts as non-finite; x*x (exact in fp64) is added in fp64 per
 *              thread in grid-stride order, then over the 64 lanes (l += l+32, l+16, ... l+1), then over the 4 waves in
 *              order; one {sumsq, nonfinite} per block goes to `ws` (dyk_grad_stats_ws_bytes(n) bytes, 16-byte aligned)
 *   finalize : one workgroup adds the block partials in block-index order in fp64 and one lane writes the record:
 *              norm = fl32(sqrt(sumsq));  c = max_norm / (norm + 1e-6f) in fp32;
 *              coef = max_norm > 0 ? (c > 1 ? 1 : c) : 1      (torch's clip_grad_norm_; a NaN norm gives a NaN coef, as
 *                                                              with error_if_nonfinite=False)
 *              skip = skip_nonfinite && nonfinite > 0
 *              !skip: applied += 1, bc1 = fl32(1 - beta1^applied), bc2_sqrt = fl32(sqrt(1 - beta2^applied)), both formed
 *              in double as dyk_adam_step forms them from `step`;  skip: skipped += 1 (bc1, bc2_sqrt keep their values)
 *   The record lives in device memory owned by the caller and is kept across steps (applied / skipped are read and
 *   written); zero it once.  No atomics, no in-launch hand-off: the kernel boundary orders partials before finalize.
 * dyk_adam_step_guarded / dyk_sgd_step_guarded : dyk_adam_step / dyk_sgd_step with the decision taken from the record:
 *   rec->skip != 0 : g is cleared when zero_grad is set; p, m, v, wc keep their bits
 *   otherwise      : the same statements with grad_scale := fl32(desc.grad_scale * rec->coef), the bias corrections
 *                    rec->bc1 / rec->bc2_sqrt instead of those of desc.step (which is ignored), and SGD's first-step rule
 *                    (m = g') when rec->applied == 1.  Same contracts as DykOptimDesc above; the desc may name a sub-range.
 * dyk_grad_scale_by_rec : g[i] = fl32(g[i] * rec->coef) on live elements; nothing is stored when rec->coef == 1.0f.
 * n a positive multiple of 4; g 16-byte, ws 16-byte, rec 8-byte, mask 4-byte aligned; otherwise (or with a NULL g / ws / rec
 * or ws_bytes < dyk_grad_stats_ws_bytes(n)) DYK_ERR_ARG before any launch.
 * ---------------------------------------------------------------------------------- */
typedef struct DykGradGuardRec {
    double sumsq;          /* sum of x*x over the live elements */
    float norm;            /* fl32(sqrt(sumsq)) */
    float coef;            /* clip coefficient (1 when max_norm <= 0) */
    uint32_t nonfinite;    /* live elements that are inf / NaN (saturates at 2^32 - 1) */
    int32_t skip;          /* 1: the step that follows leaves p, m, v, wc alone */
    int32_t applied;       /* steps taken so far (Adam's t) */
    int32_t skipped;       /* steps skipped so far */
    float bc1, bc2_sqrt;   /* bias corrections at t = applied */
} DykGradGuardRec;
typedef struct DykGradStatsDesc {
    const float* g;
    const uint8_t* mask;   /* NULL or one byte per element, 0 = frozen (not counted, not summed) */
    void* ws;
    DykGradGuardRec* rec;
    int64_t n;
    int64_t ws_bytes;
    float grad_scale;
    float max_norm;        /* <= 0: no clipping (coef = 1) */
    float beta1, beta2;    /* for bc1 / bc2_sqrt (SGD: unused by the step, any value in [0, 1)) */
    int32_t skip_nonfinite;
    int32_t _pad;
} DykGradStatsDesc;
int64_t dyk_grad_stats_ws_bytes(int64_t n);
int dyk_grad_stats(const DykGradStatsDesc* desc, void* stream);
int dyk_adam_step_guarded(const DykOptimDesc* desc, const DykGradGuardRec* rec, void* stream);
int dyk_sgd_step_guarded(const DykOptimDesc* desc, const DykGradGuardRec* rec, void* stream);
int dyk_grad_scale_by_rec(float* g, const uint8_t* mask, int64_t n, const DykGradGuardRec* rec, void* stream);

/* ------------------------------------------------------------------------------------
 * Parameter groups and decoupled weight decay for the fused optimizer steps (the YOLOv3/v4 recipe behind the reference's
 * hyp.scratch*.json: weight decay on convolution weights only, a learning rate of their own for the biases during warm-up,
 * AdamW), still one launch over the flat buffers.  The mask byte of DykOptimDesc carries the group:
 *   0                          : frozen parameter or padding -- no update, no decay, moments untouched, g cleared when zero_grad
 *                                is set (the meaning it has for dyk_adam_step / dyk_sgd_step)
 *   k in 1..groups->count      : the element belongs to group k-1 and is updated with groups->g[k-1]
 *   k > groups->count          : treated as 0 (frozen)
 * Parameters start at multiples of 64 elements, so the four bytes of a 16-byte vector agree; the kernels read them as one
 * 32-bit word and take its low byte.  "Live" keeps the meaning it has for dyk_grad_stats and dyk_grad_scale_by_rec (the four
 * mask bytes not all 0): both take a group map as their mask unchanged.
 * DykOptimGroups is passed to the kernel BY VALUE, as a kernel argument: a scheduler changes lr at every step, and a table in
 * device memory would need a copy and an ordering edge per step.
 *   lr, weight_decay : of the group; desc->lr and desc->weight_decay are ignored
 *   flags bit 0      : DYK_OPT_GROUP_DECOUPLED, decoupled weight decay (torch.optim.AdamW): p = fl32(p * decay_mul) first, then
 *                      the Adam statements with weight_decay = 0.  Without it: L2, the statements of dyk_adam_step / dyk_sgd_step
 *                      with the group's lr and weight_decay.  Other bits must be 0.
 *   decay_mul        : fl32(1 - fl32(lr * weight_decay)), formed by the caller; read for decoupled groups only
 * beta1, beta2, eps (SGD: momentum in beta1), grad_scale, step, zero_grad and wc stay in DykOptimDesc and are shared by all
 * groups.  The per-element statements are those of dyk_adam_step / dyk_sgd_step (one device function, csrc/optim.hip): a
 * group without the decoupled flag gets the bits dyk_adam_step / dyk_sgd_step give with that group's lr and weight_decay.
 * dyk_adam_step_groups / dyk_sgd_step_groups(desc, groups, rec, stream):
 *   rec == NULL : as dyk_adam_step / dyk_sgd_step -- bias corrections from desc->step (>= 1), SGD's first-step rule at step == 1
 *   rec != NULL : as the _guarded entries -- rec->skip, grad_scale := fl32(desc->grad_scale * rec->coef), rec->bc1 /
 *                 rec->bc2_sqrt, and the first-step rule at rec->applied == 1 (desc->step is ignored)
 * The desc may name a sub-range (mask offset with it).  Before any launch: everything dyk_adam_step / dyk_sgd_step check, and
 * mask not NULL and 4-byte aligned, 1 <= count <= DYK_OPT_MAX_GROUPS, every lr finite, every weight_decay >= 0, no unknown
 * flag bit, rec 8-byte aligned; otherwise DYK_ERR_ARG and nothing is written.  A decoupled group handed to
 * dyk_sgd_step_groups: DYK_ERR_UNSUPPORTED, nothing written.
 * ---------------------------------------------------------------------------------- */
#define DYK_OPT_MAX_GROUPS 8
#define DYK_OPT_GROUP_DECOUPLED 1
typedef struct DykOptimGroup {
    float lr;
    float weight_decay;
    float decay_mul;
    uint32_t flags;
} DykOptimGroup;
typedef struct DykOptimGroups {
    int32_t count;
    int32_t _pad[3];
    DykOptimGroup g[DYK_OPT_MAX_GROUPS];
} DykOptimGroups;
int dyk_adam_step_groups(const DykOptimDesc* desc, const DykOptimGroups* groups, const DykGradGuardRec* rec_or_null, void* stream);
int dyk_sgd_step_groups(const DykOptimDesc* desc, const DykOptimGroups* groups, const DykGradGuardRec* rec_or_null, void* stream);

/* ------------------------------------------------------------------------------------
 * Exponential moving average of the flat buffers (replaces the per-entry loop of ModelEMA.update, reference
 * build_utils/torch_utils.py:108-120: `v *= d; v += (1. - d) * msd[k]` over every floating state_dict entry).
 * One launch for up to DYK_EMA_MAX_REGIONS regions (the parameter store P and the running statistics R):
 *   dst[r][i] = fl32(fl32(dst[r][i] * d) + fl32(omd * src[r][i]))    i < n[r]
 * two roundings per product and one per sum, no FMA: bit-identical to torch's fp32 ops, NaN / Inf included.
 *   d   : the decay rounded to fp32;  omd : (1 - decay) formed in double, then rounded to fp32
 * Every n[r] a positive multiple of 4, every pointer 16-byte aligned, 1 <= nregions <= DYK_EMA_MAX_REGIONS; otherwise
 * DYK_ERR_ARG before any launch.
 * ---------------------------------------------------------------------------------- */
#define DYK_EMA_MAX_REGIONS 4
typedef struct DykEmaDesc {
    const float* src[DYK_EMA_MAX_REGIONS];   /* the live model's buffers (read) */
    float* dst[DYK_EMA_MAX_REGIONS];         /* the shadow's buffers (read, written) */
    int64_t n[DYK_EMA_MAX_REGIONS];
    int32_t nregions;
    float d, omd;
} DykEmaDesc;
int dyk_ema_update(const DykEmaDesc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * Per-tensor statistics of up to DYK_TSTAT_MAX_BUFS flat fp32 buffers that share one segment table (the parameter store P,
 * its gradient G and the fused optimizers' flat moments; replaces a host loop of `p.grad.norm()` / `torch.isfinite(p.grad)`
 * over some 600 views, each with its own kernels and a `.item()` synchronisation).  A segmented reduction in two launches; no
 * atomics and no in-launch hand-off: the kernel boundary orders the partials before the fold.
 *
 * Segment s is the elements [offset, offset + numel) of every buffer: offset a multiple of 4 (16-byte vector loads hold; the
 * parameter store gives multiples of 64), numel >= 1 and NOT necessarily a multiple of 4.  What lies between segments is never
 * read into any field (the 16-byte vector that holds a segment's last elements is loaded whole and masked per element).
 * flags bit k (k < nbuf) : segment s is skipped for buffer k -- buf[k] is not read there and out[s][k] is written as all zeros
 * (frozen parameters have neither gradient nor moments).
 * The work list cuts every segment, in table order, into items of DYK_TSTAT_ITEM = 4096 elements (the last one shorter):
 *   item i = {first = offset + 4096 * j, seg = s, len}  for j = 0 .. ceil(numel / 4096) - 1,   seg[s].item_begin = index of j = 0
 * It is a function of the table only; the caller builds it once per table and keeps both on the device (dyk.ops.
 * tensor_stats_worklist).  An item never crosses a segment.
 *
 * Per (segment, buffer) -- DykTensorStat:
 *   sumsq     : sum of x*x over the FINITE elements, in fp64.  Each x*x is exact in fp64 (two 24-bit significands); a
 *               non-finite element contributes an exact 0.
 *   absmax    : max of |x| over the finite elements, 0 when there is none.  Exact.
 *   nonfinite : elements with !(|x| <= FLT_MAX) (inf, NaN).  Exact; saturates at 2^32 - 1.
 *   zeros     : elements equal to +0.0 or -0.0.  Exact; saturates at 2^32 - 1.
 *
 * dyk_tensor_stats : two launches on `stream`:
 *   partials : one workgroup of 256 threads per item (grid = nitems), all nbuf buffers in the same pass.  Thread t takes the
 *              16-byte vectors t, t + 256, t + 512, t + 768 of the item, in that order, and the four elements of a vector in
 *              order; elements at or past `len` are left out.  Per buffer the thread adds x*x (0 for a non-finite x) to an
 *              fp64 accumulator that starts at +0.0, one fused multiply-add per element (one rounding: the product is exact).
 *              The 64 lanes of a wave fold as l += l+32, l+16, l+8, l+4, l+2, l+1; the four waves add in order
 *              ((w0 + w1) + w2) + w3.  One partial {sumsq, absmax, nonfinite, zeros} per (item, buffer) goes to
 *              ws[item * nbuf + k] (dyk_tensor_stats_ws_bytes(nitems, nbuf) bytes, 8-byte aligned).
 *   fold     : one wave per segment (workgroups of 4 waves, grid = ceil(nseg / 4)).  With b = seg[s].item_begin and
 *              c = ceil(numel / 4096), lane l adds the partials b + l, b + l + 64, b + l + 128, ... (< b + c) in that order to
 *              an accumulator that starts at +0.0; the lanes fold as above; lane 0 writes out[s * nbuf + k].
 *   Every addition adds values >= 0, so adding the exact zeros of absent elements / partials changes no bit: sumsq is a
 *   function of (buffers, table) only, bit-identical from run to run and independent of grid size and arrival order, and a
 *   restatement that performs these additions in this order (tests/tensor_stats_ref.py) reproduces it bit for bit.
 *   absmax and the counts are exact in any order.
 * Argument contract: buf[0..nbuf) 16-byte aligned, each of n elements, n a positive multiple of 4; every segment inside
 * [0, n); seg, items, ws and out 8-byte aligned; 1 <= nbuf <= DYK_TSTAT_MAX_BUFS; nseg >= 1; nitems >= nseg;
 * ws_bytes >= dyk_tensor_stats_ws_bytes(nitems, nbuf).  Otherwise (or with a NULL descriptor / buffer / table / work list /
 * workspace / output) DYK_ERR_ARG before any launch.  The tables live in device memory, so the kernels check them: an item
 * that names a segment outside the table, is longer than 4096, does not lie inside its segment or inside [0, n), and a
 * segment whose items do not lie inside the work list, read nothing and contribute zeros.
 * dyk_tensor_stats_ws_bytes(nitems, nbuf) : bytes of workspace, 0 for arguments out of range.
 * ---------------------------------------------------------------------------------- */
#define DYK_TSTAT_MAX_BUFS 4
#define DYK_TSTAT_ITEM 4096
typedef struct DykTensorSeg {
    int64_t offset;        /* first element, a multiple of 4 */
    int64_t numel;         /* >= 1 */
    uint32_t flags;        /* bit k: skipped for buffer k */
    int32_t item_begin;    /* index of the segment's first item in the work list */
} DykTensorSeg;
typedef struct DykTensorItem {
    int64_t first;         /* first element of the item in the buffers (seg.offset + 4096 * j) */
    int32_t seg;
    int32_t len;           /* 1 .. 4096 */
} DykTensorItem;
typedef struct DykTensorStat {
    double sumsq;
    float absmax;
    uint32_t nonfinite;
    uint32_t zeros;
    uint32_t _pad;         /* written as 0 */
} DykTensorStat;
typedef struct DykTensorStatsDesc {
    const float* buf[DYK_TSTAT_MAX_BUFS];
    const DykTensorSeg* seg;       /* device, [nseg] */
    const DykTensorItem* items;    /* device, [nitems] */
    void* ws;                      /* device, dyk_tensor_stats_ws_bytes(nitems, nbuf) bytes */
    DykTensorStat* out;            /* device, [nseg][nbuf] */
    int64_t n;                     /* elements of every buffer */
    int64_t ws_bytes;
    int32_t nbuf;
    int32_t nseg;
    int32_t nitems;
    int32_t _pad;
} DykTensorStatsDesc;
int64_t dyk_tensor_stats_ws_bytes(int64_t nitems, int32_t nbuf);
int dyk_tensor_stats(const DykTensorStatsDesc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * Stem convolution (Cin = 3, 3x3, pad 1, stride 1 | 2, Cout 16 | 32) straight from the image batch, no im2col.
 * Replaces `imgs.float() / 255.0` (train_utils/kaist_train_eval_utils.py:54-55, evaluate.py:67-68) + nn.Conv2d(3, C, 3)
 * of module_list[0] / module_list[second_index] (models.py:34-42) and that layer's weight gradient.
 *   img  : [B][3][H][W] NCHW, float32 in 0..1, or uint8 (in_u8 != 0: each value is divided by 255.0f on the fly, the
 *          same fp32 quotient the reference's `.float() / 255.0` produces)
 *   fwd  : y[b, yo, xo, co] = sum_{ky,kx,c} img[b, c, yo*stride-1+ky, xo*stride-1+kx] * w[co][ky][kx][c]  (fp32 FMAs),
 *          wt = the same weights transposed to [27][Cout] fp32; raw output + per-channel sum / sum of squares into a
 *          `stats` replica (training), or act(y*scale + shift) when scale != NULL (eval: folded BatchNorm)
 *   wgrad: dw[co][(ky*3+kx)*3 + c] += sum over pixels dy * img, on the fp32-input MFMA; `part` = workspace of
 *          dyk_stem_wgrad_planes(desc) * Cout * 27 floats (per-wave partial tiles, folded in a fixed order)
 * ---------------------------------------------------------------------------------- */
typedef struct DykStemDesc {
    const void* img;
    const float* wt;       /* [27][Cout] (forward) */
    void* y;               /* forward output, dtype, rows of ldy elements */
    double* stats;         /* [stats_slots][2*Cout] or NULL */
    const float* scale;    /* [Cout] or NULL */
    const float* shift;    /* [Cout] or NULL */
    const void* dy;        /* wgrad: gradient wrt y, dtype, rows of lddy elements */
    float* dw;             /* wgrad: [Cout][27], accumulated */
    float* part;           /* wgrad workspace */
    /* wgrad with bn_fused != 0 (uint8 images, bf16): the BatchNorm-backward APPLY pass of the stem's own BatchNorm is done on
     * the fly instead of by a separate dyk_bn_act_bwd_apply launch -- `dy` is not read; the kernel reads da (the gradient wrt the
     * normalised output with act' already applied, as a fused data-gradient epilogue leaves it) and the raw conv output, folds
     * the two reduction sums from the replicas and feeds  dz = scale * (da - S1/N - xhat * S2/N),  xhat = (yraw - mean) * rstd,
     * rounded to bf16 as the apply pass would store it, to the weight gradient; workgroup 0 adds S2 / S1 to dgamma / dbeta.
     * Saves one pass over the largest activation of the net (512 x 640 x 32 per image): written once less, read once less. */
    const void* bn_da;     /* [B,Ho,Wo,Cout] dtype, rows of Cout elements */
    const void* bn_yraw;   /* raw conv output, same layout */
    const float* bn_vecs;  /* scale | shift | mean | rstd, Cout floats each */
    const double* bn_red;  /* [bn_slots][2][Cout]: sum(da), sum(da * xhat) replicas */
    float* bn_dgamma;      /* += S2 (or NULL) */
    float* bn_dbeta;       /* += S1 (or NULL) */
    int32_t dtype, in_u8;
    int32_t B, H, W, Cout, k, stride, pad, Ho, Wo;
    int32_t ldy, lddy, act, stats_slots;
    int32_t bn_fused, bn_slots;
} DykStemDesc;
int dyk_stem_conv_fwd(const DykStemDesc* desc, void* stream);
int dyk_stem_conv_wgrad(const DykStemDesc* desc, void* stream);
int dyk_stem_wgrad_planes(const DykStemDesc* desc);
/* 1 when dyk_stem_conv_wgrad would accept `desc` with bn_fused set (its bn_* fields and in_u8 / img filled in): the caller then
 * sets bn_fused and DYK_EW_SKIP on the BatchNorm's own dyk_bn_act_bwd_apply descriptor; 0: run the two passes separately. */
int dyk_stem_wgrad_bn_fusable(const DykStemDesc* desc);

/* Dependency-scheduled execution on several HIP streams.  The plan compiler derives the read / write sets of every
 * command from its descriptor, builds the dependency graph and list-schedules it onto n_streams in-order streams
 * (dyk/sched.py); this entry point replays the result.  Entries are in ISSUE order.  Entry k launches command
 * cmds[sched[k].cmd] on stream sched[k].stream (0 = the caller's `stream`, 1.. = library-owned streams) after making
 * that stream wait for the completion events of the entries sched[k].wait[0..nwait) (positions < k, always on other
 * streams), and records a completion event afterwards when `record` is set.  On entry every library stream waits for
 * what the caller's stream holds so far; on return the caller's stream waits for all of them.  No host synchronisation.
 * low_priority_last != 0: the last stream is created with the lowest priority (filler work such as weight gradients). */
typedef struct DykSchedEntry {
    int32_t cmd;
    int16_t stream;
    int8_t nwait;
    int8_t record;
    int32_t wait[7];
    int32_t cmd2;         /* >= 0: cmds[cmd] and cmds[cmd2] are a shape-identical, mutually independent pair (the twin backbones):
                             enqueued as ONE two-problem launch (dyk_run_command_pair); < 0: none */
} DykSchedEntry;
int dyk_run_schedule(const DykCommand* cmds, const DykSchedEntry* sched, int32_t n_entries, int32_t n_streams,
                     int32_t low_priority_last, void* stream, int32_t* failed_index);
/* A command range as a hipGraph built from dependency lists: command i depends on commands dep_idx[dep_off[i] ..
 * dep_off[i+1]) (all < i).  Each command is captured alone (single-stream capture) into a child graph node of the master
 * graph; the instantiated graph is launched with one host call per pass.  Kernel arguments -- every pointer inside the
 * descriptors -- are frozen at capture; capture again when one changes.  *graph_out is an opaque handle. */
int dyk_dag_graph_create(const DykCommand* cmds, int32_t n, const int32_t* dep_off, const int32_t* dep_idx,
                         void** graph_out, int32_t* failed_index);
int dyk_schedule_graph_launch(void* graph, void* stream);
int dyk_schedule_graph_destroy(void* graph);

/* ------------------------------------------------------------------------------------
 * Box-coordinate helpers of the evaluation chain (build_utils/utils.py:40-92; callers evaluate.py:82,
 * detect.py:114).  Rows of `ld` floats, the first four columns are the box.  fp32, rounded exactly like the
 * reference's torch-CPU expressions.
 *   dyk_box_convert : to_xyxy != 0: (xc,yc,w,h) -> (x1,y1,x2,y2) [xywh2xyxy :50-57]; else the inverse
 *                     [xyxy2xywh :40-47].  in may equal out.
 *   dyk_scale_coords: in place.  do_scale != 0: x = (x - pad_x) / gain, y = (y - pad_y) / gain [scale_coords
 *                     :60-81] and then, always, clamp x to [0, w0], y to [0, h0] [clip_coords :84-92].
 * ---------------------------------------------------------------------------------- */
int dyk_box_convert(const float* in, float* out, int32_t n, int32_t ld_in, int32_t ld_out, int32_t to_xyxy, void* stream);
int dyk_scale_coords(float* boxes, int32_t n, int32_t ld, float pad_x, float pad_y, float gain, float w0, float h0,
                     int32_t do_scale, void* stream);

/* ------------------------------------------------------------------------------------
 * Matching of one evaluation batch's detections to its ground truth, per class and per IoU threshold (replaces the
 * per-batch half of the evaluation: other_utils/metrics.py box_iou :62-79 and the matching loop of compute_ap_lamr
 * :81-130, the caller's loop evaluate.py:76-106, scale_coords / clip_coords build_utils/utils.py:60-92).  One launch,
 * one wavefront per image, no allocation, no atomics, no synchronisation; the curve arithmetic (once per epoch) stays
 * on the host (other_utils.metrics.compute_map).
 *
 * Reads   out [B][max_num][6] (x1,y1,x2,y2,conf,cls) and counts [B] as dyk_nms leaves them (counts[b] <= 0: no detection),
 *         rec_off [B]   first record of image b; records [rec_off[b], rec_off[b] + counts[b]) must lie inside rec_cap,
 *         targets [nt][6] (image in batch, class, xc, yc, w, h; relative), sorted by image: image b owns rows
 *         [gt_off[b], gt_off[b+1]), at most DYK_EVAL_MAX_GT of them,
 *         shape0 [B][2] original (width, height), unpad [B][4] (pad_x, pad_y, gain, do_scale) or NULL (boxes as they are).
 * Per image, type for type the arithmetic of the host evaluator, so every decision is the same decision:
 *   ground truth  fp32, no FMA: x *= w0, y *= h0, x1 = xc - w / 2, x2 = w + x1 (likewise y), truncated to int32;
 *   detections    do_scale != 0: (x - pad) / gain, clamped to [0, w0] / [0, h0] -- the expressions of dyk_scale_coords;
 *   IoU           pixel-inclusive (+1); detection area in fp32, ground-truth area in int32, everything else in fp64
 *                 after exact conversion: extents, clip to [0, 1e5], product, inter / (a1 + a2 - inter).
 * Detections are walked in NMS order.  For detection d of class c: k = the box of class c in the image with the largest
 * IoU, the lowest index among equals (np.argmax); for every threshold t: tp_t = iou >= thr[t] && !claimed_t[k], and a true
 * tp_t claims k at t.  A best box that is already claimed makes d a false positive at t (no second choice).  No box of
 * class c in the image: tp_mask 0, match -1, iou 0.  A class outside [0, nc): the same record and err[0] = 1.  An image
 * whose table entries are out of range (records outside rec_cap, rows outside nt, more than DYK_EVAL_MAX_GT rows) writes
 * nothing and sets err[1] = 1.  err [2] is only ever set, with plain stores of the same word; the caller clears it.
 * Writes, per detection r = rec_off[b] + rank: conf[r], cls[r], tp_mask[r] (bit t), match[r] (row of `targets` or -1),
 * iou[r] (the best one, fp64), box[r][4] (the box the IoU was taken of).
 * DYK_ERR_ARG before any launch: a null pointer (unpad and targets with nt == 0 excepted), B < 1, max_num < 1, nc < 1,
 * T outside [1, DYK_EVAL_MAX_THR], nt < 0, rec_cap < 0.
 * ---------------------------------------------------------------------------------- */
#define DYK_EVAL_MAX_THR 16
#define DYK_EVAL_MAX_GT 1024
typedef struct DykEvalMatchDesc {
    const float* out;
    const int32_t* counts;
    const int32_t* rec_off;
    const float* targets;
    const int32_t* gt_off;
    const int32_t* shape0;
    const float* unpad;
    float* conf;
    int32_t* cls;
    uint32_t* tp_mask;
    int32_t* match;
    double* iou;
    float* box;
    int32_t* err;
    double thr[DYK_EVAL_MAX_THR];
    int32_t B, max_num, nt, nc, T, rec_cap;
} DykEvalMatchDesc;
int dyk_eval_match(const DykEvalMatchDesc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * COCO-protocol matching of one evaluation batch (replaces the per-batch half of the training harness's validation,
 * train_utils/kaist_train_eval_utils.py:122-190: scale_coords + round per image, three device-to-host copies, a dict
 * per detection, then pycocotools' per-image evaluation).  One launch, one workgroup (a wavefront) per image, no
 * allocation, no atomics, no synchronisation; the accumulation (once per epoch) stays on the host
 * (other_utils.metrics.coco_accumulate).  Written from the published algorithm; no COCO tool runs where this project
 * runs, so agreement with pycocotools is derived (this text, tests/coco_ref.py and its hand cases), not measured.
 *
 * Inputs as dyk_eval_match reads them (out, counts, rec_off, targets, gt_off, shape0, unpad), plus area[a] = [lo, hi]
 * for a < A, max_det, round_boxes, img_base.  Every step is a separate IEEE operation, no FMA:
 *   ground truth  fp32: gx = (xc - 0.5f*w) * (float)W0, gy = (yc - 0.5f*h) * (float)H0, gw = w * (float)W0,
 *                 gh = h * (float)H0 (coco_utils.py:33-45 on an fp32 tensor); then exactly to fp64, garea = gw * gh.
 *   detections    un-letterboxed and clipped with the expressions of dyk_scale_coords when unpad says so; round_boxes
 *                 != 0: rintf (half to even) on each corner (kaist_train_eval_utils.py:163); dw = x2 - x1, dh = y2 - y1
 *                 in fp32; then fp64, darea = dw * dh.
 *   IoU           fp64: w = min(dx+dw, gx+gw) - max(dx, gx), w <= 0 -> 0; h likewise; i = w*h; i / (darea + garea - i).
 *                 No +1 anywhere.
 *   rank          within the image and the class value: #{j of the class : s_j > s_i || (s_j == s_i && j < i)} (a stable
 *                 descending sort); ranks >= max_det take no part in the matching.
 *   per area a    a ground-truth box is ignored when garea < lo || garea > hi; the boxes of the class are visited
 *                 non-ignored first, then ignored, each group in row order.
 *   per (a, t)    detections in rank order: best = min(thr[t], 1 - 1e-10), m = none; walk the boxes in visiting order:
 *                 skip a box matched at (a, t); stop when m is a non-ignored box and the next one is ignored; skip a box
 *                 with iou < best; otherwise best = iou, m = this box (on equal IoU the later box wins).  With an m the
 *                 detection is matched, its ignore flag is m's, and m is matched at (a, t); without one the detection is
 *                 ignored exactly when darea < lo || darea > hi.
 * Writes, per detection r = rec_off[b] + i in NMS order: conf[r], cls[r], img[r] = img_base + b, rank[r], box[r][4] (the
 * corners as used), darea[r], dtm[r][A] / dtig[r][A] (bit t: matched / ignored at (a, t)), match[r][A][T] (index of the
 * matched box among the image's rows of `targets`, -1 if none).  A detection with rank >= max_det, or with a class outside
 * [0, nc) (then err[0] = 1), gets zeros in dtm and dtig and -1 in every match.  Tables that leave the arrays, or more than
 * DYK_EVAL_MAX_GT rows: the image writes nothing and err[1] = 1, as in dyk_eval_match.
 * DYK_ERR_ARG before any launch: the causes of dyk_eval_match, A outside [1, DYK_EVAL_MAX_AREA], A * T > 64 (one lane
 * decides one (a, t)), max_det < 1, max_num > DYK_EVAL_COCO_MAX_NUM (the detections of an image are ranked in LDS; the
 * NMS entry points keep at most that many).
 * ---------------------------------------------------------------------------------- */
#define DYK_EVAL_MAX_AREA 4
#define DYK_EVAL_COCO_MAX_NUM 512
typedef struct DykEvalCocoDesc {
    const float* out;
    const int32_t* counts;
    const int32_t* rec_off;
    const float* targets;
    const int32_t* gt_off;
    const int32_t* shape0;
    const float* unpad;
    float* conf;
    int32_t* cls;
    int32_t* img;
    int32_t* rank;
    float* box;
    double* darea;
    uint32_t* dtm;
    uint32_t* dtig;
    int16_t* match;
    int32_t* err;
    double thr[DYK_EVAL_MAX_THR];
    double area[DYK_EVAL_MAX_AREA][2];
    int32_t B, max_num, nt, nc, T, rec_cap;
    int32_t A, max_det, round_boxes, img_base;
} DykEvalCocoDesc;
int dyk_eval_match_coco(const DykEvalCocoDesc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * The "snowflake" input transform on the device (reference build_utils/snowflake.py: contrast-limited adaptive histogram
 * equalisation of every channel of both streams, then square cut-outs): dyk_clahe and dyk_cutout_rects.
 *
 * dyk_clahe is OpenCV's 8-bit CLAHE (modules/imgproc/src/clahe.cpp), per plane of src[planes][H][W].  Written from the
 * published algorithm; no OpenCV runs where this project runs, so agreement with it is derived (this text,
 * tests/clahe_ref.py and its hand cases), not measured.  The rule:
 *   geometry      W % tiles_x == 0 && H % tiles_y == 0: padx = pady = 0.  Otherwise padx = tiles_x - W % tiles_x and
 *                 pady = tiles_y - H % tiles_y -- a divisible axis then gets a full extra tiles_x / tiles_y (OpenCV does so).
 *                 The tiles cover the image extended by BORDER_REFLECT_101 (index j >= n reads 2(n-1) - j), read through
 *                 the index map, never materialised.  tw = (W+padx)/tiles_x, th = (H+pady)/tiles_y, area = tw*th.
 *   constants     lutScale = 255.0f / (float)area in fp32;
 *                 clip = clip_limit > 0 ? max((int)(clip_limit * area / 256), 1) : 0, product and quotient in double.
 *   per tile      1. the 256-bin int histogram of its tw x th extended pixels;
 *                 2. if clip > 0: clipped = sum(max(h - clip, 0)), every bin becomes min(h, clip); batch = clipped / 256,
 *                    residual = clipped - 256*batch; every bin += batch; if residual != 0: step = max(256 / residual, 1) and
 *                    the bins 0, step, 2*step, ... get +1 each while the index is < 256 and fewer than `residual` bins
 *                    have been incremented;
 *                 3. lut[i] = saturate_u8(rint_half_even((float)prefix_sum_i * lutScale)), prefix sum inclusive.
 *   per pixel     (y, x) of the original H x W, v = src: txf = x * (1.0f/tw) - 0.5f, tx1 = floor(txf), xa = txf - tx1,
 *                 xa1 = 1.0f - xa; then tx1 is clamped at 0 and tx2 = tx1 + 1 (of the unclamped tx1) at tiles_x - 1 -- the
 *                 clamping comes after xa is formed; the same in y.  With L[ty][tx] the table of tile (ty, tx):
 *                 res = (L[ty1][tx1][v]*xa1 + L[ty1][tx2][v]*xa)*ya1 + (L[ty2][tx1][v]*xa1 + L[ty2][tx2][v]*xa)*ya,
 *                 dst = saturate_u8(rint_half_even(res)).
 *   fp32          every multiply, add and subtract above is an IEEE fp32 operation rounded on its own, in exactly this
 *                 order, no FMA: plain numpy reproduces the output bit for bit.
 * Two launches on `stream` (tables, then pixels), no allocation, no synchronisation.  `lut` is the workspace
 * [planes][tiles_y*tiles_x][256] of dyk_clahe_ws_bytes(planes, tiles_x, tiles_y) = planes*tiles_x*tiles_y*256 bytes (a
 * negative DYK_ERR_ARG for planes < 1 or a grid outside 1..16); it holds the tables afterwards.  dst == src is allowed: a
 * pixel reads only its own source byte.  Any alignment works; 4-byte aligned src / dst with W % 4 == 0 and a 16-byte
 * aligned lut take the vector paths.
 * DYK_ERR_ARG before any launch: a null pointer; planes, H or W < 1; tiles_x / tiles_y outside 1..16; a pad larger than
 * n - 1 on its axis (the reflection is undefined); area > 2^24 (above it (float)prefix_sum stops being exact);
 * planes * max(H, 256) > INT32_MAX (one grid dimension).
 *
 * dyk_cutout_rects: plane p of img[planes][H][W] uses the rectangle set p / planes_per_set of
 * rects[nsets][nrect][4] = (xmin, ymin, xmax, ymax), in device memory; rows [ymin, ymax) and columns [xmin, xmax) are set to
 * `value` -- the upper ends are exclusive, as in the reference's slices (snowflake.py:88-91).  Rectangles are clipped to the
 * image; empty or inverted ones write nothing.  One launch for all planes; nrect == 0 launches nothing.
 * DYK_ERR_ARG: null img, null rects with nrect > 0, planes / H / W / planes_per_set < 1, nrect < 0, value outside 0..255,
 * H*W or planes*nrect > INT32_MAX.
 * ---------------------------------------------------------------------------------- */
typedef struct DykClaheDesc {
    const uint8_t* src;   /* [planes][H][W] */
    uint8_t* dst;         /* [planes][H][W]; dst == src allowed */
    uint8_t* lut;         /* workspace [planes][tiles_y*tiles_x][256] */
    int32_t planes, H, W, tiles_x, tiles_y;
    double clip_limit;    /* <= 0: no clipping */
} DykClaheDesc;
int64_t dyk_clahe_ws_bytes(int32_t planes, int32_t tiles_x, int32_t tiles_y);
int dyk_clahe(const DykClaheDesc* desc, void* stream);
int dyk_cutout_rects(uint8_t* img, int32_t planes, int32_t H, int32_t W, const int32_t* rects, int32_t nrect,
                     int32_t planes_per_set, int32_t value, void* stream);

/* ------------------------------------------------------------------------------------
 * The random training augmentation of image pairs on the device (reference build_utils/kaist_dataset.py:213-286 mosaic,
 * :408-479 random_affine, :482-506 augment_hsv, :362-369 flip): dyk_augment_pairs, ONE launch for both streams of a batch.
 * The draws and the label arithmetic stay on the host (build_utils/augment.py); every pixel is made here.
 *
 * The rule is the classical OpenCV 8-bit path -- warpAffine(INTER_LINEAR, BORDER_CONSTANT 0), then cvtColor BGR2HSV, three
 * table look-ups, cvtColor HSV2BGR -- written down as this project's own rule.  It is DERIVED, NOT MEASURED: no OpenCV runs
 * where this project runs, and newer OpenCV releases changed their warp kernels; what is held bit for bit is this text,
 * tests/augment_ref.py and its hand-worked cases.  Per output pixel the stages run in the order warp, HSV, flipped store.
 *
 * (a) Virtual canvas.  Output image b samples a canvas of Hc x Wc pixels made of up to four disjoint rectangles, int32
 *     records rects[b][4][8] = (x1, y1, x2, y2, src, dx, dy, pad), upper ends exclusive:
 *         canvas(b, c, y, x) = src_img[src][c][y - dy][x - dx]   when (x, y) lies inside a rectangle (the first that holds it),
 *                              0                                  everywhere else, outside the canvas included.
 *     The mosaic's background and the warp's border value are both 0: one rule.  A rectangle is clipped to the canvas; one
 *     that is empty, names a src outside 0..N-1 or reaches outside its source image is skipped whole (the kernel never reads
 *     outside src; the Python wrapper refuses such rectangles).  rects == NULL: the one rectangle (0, 0, W, H, b, 0, 0) on a
 *     canvas of H x W.
 * (b) Warp.  minv[b][6] is the INVERSE map (output -> canvas), fp64.  The host inverts the forward matrix M (2 x 3) in fp64 in
 *     exactly this order: D = M0*M4 - M1*M3; D = 1/D; A11 = M4*D; A22 = M0*D; M0 = A11; M1 *= -D; M3 *= -D; M4 = A22;
 *     b1 = -M0*M2 - M1*M5; b2 = -M3*M2 - M4*M5; M2 = b1; M5 = b2.   rn = round half to even to int32, saturating.
 *         per output column x:   ad = rn(m0*x*1024),                 bd = rn(m3*x*1024)
 *         per output row y:      X0 = rn((m1*y + m2)*1024) + 16,     Y0 = rn((m4*y + m5)*1024) + 16
 *     every fp64 multiply and add rounded on its own (no fused multiply-add).  Then, with arithmetic shifts on negatives,
 *         X = (X0 + ad) >> 5;  Y = (Y0 + bd) >> 5;  sx = X >> 5;  sy = Y >> 5;  fx = X & 31;  fy = Y & 31
 *         acc = (32-fx)(32-fy)*c(sy,sx) + fx(32-fy)*c(sy,sx+1) + (32-fx)fy*c(sy+1,sx) + fx*fy*c(sy+1,sx+1)
 *         out = (acc + 512) >> 10
 *     with each tap c(y, x) = canvas(b, c, y, x) on its own: taps may straddle a seam or the border.  minv == NULL: identity
 *     (out = canvas at the same pixel).  The Python wrapper admits only finite, non-singular matrices, sizes up to 16384 and
 *     maps whose output corners, and whose column and row terms m0*(Wo-1), m3*(Wo-1), m1*(Ho-1), m4*(Ho-1), all stay below
 *     2^20 pixels in magnitude, so no rn saturates in an admitted call.  (The C entry itself admits any matrix: rn saturates
 *     and the two sums wrap as unsigned, and the canvas look-up bounds every tap.)
 * (c) HSV jitter.  Planes are R, G, B.  v = max, vmin = min, diff = v - vmin;
 *         s = (diff * sdiv[v] + 2048) >> 12
 *         h = (g - b) if v == r, else (b - r + 2 diff) if v == g, else (r - g + 4 diff)
 *         h = (h * hdiv[diff] + 2048) >> 12;  if h < 0: h += 180
 *     sdiv[i] = rn((255 << 12) / (1.0 * i)), hdiv[i] = rn((180 << 12) / (6.0 * i)) in fp64, entry 0 of each 0.  Then
 *     (h, s, v) = (luts[b][0][h], luts[b][1][s], luts[b][2][v]) and back to RGB in fp32, every operation rounded on its own:
 *         hf = h*(6.f/180.f); sf = s*(1.f/255.f); vf = v*(1.f/255.f); sector = floor(hf) (0..5 for h <= 179); f = hf - sector
 *         tab = {vf, vf*(1-sf), vf*(1-sf*f), vf*(1-sf*(1-f))}
 *         (b, g, r) = tab[{{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}[sector]];   r = g = b = vf when s == 0
 *         channel = clip(rint_half_even(x * 255.f), 0, 255)
 *     A table hue above 179 is taken as sector 5 (the tables of build_utils.augment never hold one).  luts == NULL: no jitter.
 * (d) Flip.  flip[b] != 0: the pixel computed for column x is stored at column Wo-1-x.  flip == NULL: none.
 *
 * Both streams of image b share matrix, rectangles, table and flip.  rects / minv / luts / flip are DEVICE pointers (the
 * wrapper sends them up in one small copy from pinned memory); no allocation, no synchronisation, no atomics.
 * DYK_ERR_ARG before the launch: a null descriptor or image pointer; N, B, H, W, Ho, Wo < 1 (Hc, Wc too when rects is given)
 * or any size above 16384; rects == NULL with B > N; minv == NULL with (Ho, Wo) != the canvas size (H, W without rects);
 * a dst range that overlaps a src range or the other dst -- except dst_v == src_v and dst_l == src_l exactly with minv, rects
 * and flip all NULL and B == N (jitter alone may run in place: a pixel reads only its own three bytes).
 * ---------------------------------------------------------------------------------- */
typedef struct DykAugmentDesc {
    const uint8_t* src_v;   /* [N][3][H][W] */
    const uint8_t* src_l;   /* [N][3][H][W] */
    uint8_t* dst_v;         /* [B][3][Ho][Wo] */
    uint8_t* dst_l;         /* [B][3][Ho][Wo] */
    int32_t N, B, H, W, Hc, Wc, Ho, Wo;
    const int32_t* rects;   /* [B][4][8] or NULL */
    const double* minv;     /* [B][6] or NULL */
    const uint8_t* luts;    /* [B][3][256] or NULL */
    const uint8_t* flip;    /* [B] or NULL */
} DykAugmentDesc;
int dyk_augment_pairs(const DykAugmentDesc* desc, void* stream);
/* The same launch with `rows` (1..64) output rows per workgroup instead of the built-in choice: for tools/augment_probe.py,
 * which measures that choice; the output does not depend on it.  DYK_ERR_ARG for rows outside 1..64. */
int dyk_augment_pairs_rows(const DykAugmentDesc* desc, int32_t rows, void* stream);

/* ------------------------------------------------------------------------------------
 * Resize and letterbox of image pairs on the device (reference build_utils/kaist_dataset.py:204-208 the cv2.resize of
 * load_image, build_utils/img_utils.py:5-53 letterbox, kaist_dataset.py:378-379 BGR HWC -> RGB CHW): dyk_resize_pad_pairs,
 * ONE launch for both streams of a batch.  The geometry and the label arithmetic stay on the host
 * (build_utils/letterbox.py); every pixel is made here.
 *
 * The resize rule is the classical OpenCV 8-bit resize (modules/imgproc/src/resize.cpp: INTER_LINEAR and INTER_AREA) written
 * down as this project's own rule.  It is DERIVED, NOT MEASURED: no OpenCV runs where this project runs, and OpenCV builds
 * with IPP or newer SIMD paths may differ; what is held bit for bit is this text, tests/letterbox_ref.py and its hand-worked
 * cases.
 *
 * Per output image b the two sources (visible, LWIR) share one record: the source size h x w, the resized content size
 * nh x nw, the place (top, left) of the content in the Ho x Wo output, interp (0 = LINEAR, 1 = AREA) and the two source
 * addresses.  Sources of one batch may differ in size.  layout 0: a source is planar [3][h][w] and plane c of the output comes
 * from plane c.  layout 1: a source is interleaved [h][w][3] and plane c of the output comes from channel 2 - c (cv2.imread's
 * BGR HWC becomes planar RGB).  With S the source plane of output plane c:
 *     out(b, c, y, x) = color[c]                              outside [top, top+nh) x [left, left+nw)
 *                       resized S at (y - top, x - left)      inside; a plain copy of S when nh == h and nw == w.
 *
 * Scales, both modes, per axis in fp64: inv = (double)n_dst / (double)n_src; scale = 1.0 / inv  (two roundings; not
 * n_src / n_dst).  rn = round half to even to integer.  Every float and double multiply, add and subtract is an operation of
 * its own (no fused multiply-add).
 *
 * LINEAR.  Per destination column dx: fx = (float)((dx + 0.5) * scale_x - 0.5), computed in fp64 and cast once;
 *     sx = floor(fx); fx -= sx (fp32);  if sx < 0: sx = 0, fx = 0;  if sx >= w - 1: sx = w - 1, fx = 0;
 *     a0 = rn((1.f - fx) * 2048.f); a1 = rn(fx * 2048.f);
 *     D(sy, dx) = S[sy][sx] * a0 + S[sy][sx+1] * a1  (int32);   where sx + 1 >= w:  D = S[sy][sx] * 2048.
 *   Per destination row dy: fy, sy, b0, b1 the same way but WITHOUT the two edge resets; the two tap rows are
 *     clamp(sy, 0, h-1) and clamp(sy+1, 0, h-1), the coefficients as computed.
 *     out = ( ((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2 ) >> 2
 *   (the form of OpenCV's 8-bit vertical pass; NOT (b0*D0 + b1*D1 + 2^21) >> 22).  When both axes shrink by exactly 2
 *   (w == 2*nw and h == 2*nh) LINEAR is AREA, as in OpenCV.
 *
 * AREA, admitted only when nw <= w and nh <= h.
 *   (i) w % nw == 0 and h % nh == 0, kx = w / nw, ky = h / nh: sum = int32 sum of the kx x ky block;
 *       kx == ky == 2: out = (sum + 2) >> 2;  otherwise out = sat_u8(rn(sum * (1.f / (kx*ky)))), the reciprocal formed in fp32,
 *       one fp32 multiply.
 *   (ii) otherwise the weighted form.  Per axis and destination index d, in fp64: f1 = d * scale; f2 = f1 + scale;
 *       cell = min(scale, n_src - f1); s1 = ceil(f1); s2 = min(floor(f2), n_src - 1); s1 = min(s1, s2).  Taps, in this order:
 *           if s1 - f1 > 1e-3:  (s1 - 1, (float)((s1 - f1) / cell))
 *           for s1 <= s < s2:   (s, (float)(1.0 / cell))
 *           if f2 - s2 > 1e-3:  (s2, (float)(min(min(f2 - s2, 1.0), cell) / cell))
 *       In fp32: for each row tap (sy, beta) in order, buf = the sum over the column taps (sx, alpha) in order of
 *       (float)S[sy][sx] * alpha, starting from 0.f; acc = beta * buf for the first row tap, acc = acc + beta * buf for the
 *       following ones; out = sat_u8(rn(acc)).
 *
 * recs is a DEVICE array, read by the kernel; recs_host holds the same B records on the host and is validated before the
 * launch.  No allocation, no synchronisation, no atomics.  DYK_ERR_ARG before the launch: a null descriptor, record array,
 * destination or source pointer; B, Ho, Wo < 1; any size (B, Ho, Wo, h, w, nh, nw) above 16384; h, w, nh or nw < 1; layout or
 * interp outside their values; top < 0, left < 0, top + nh > Ho or left + nw > Wo; AREA with nw > w or nh > h; dst_v and
 * dst_l overlapping, or a destination overlapping a source.  The kernel bounds every tap by the record's h and w and never
 * reads outside a source described truthfully.
 * ---------------------------------------------------------------------------------- */
typedef struct DykResizePadRec {
    const uint8_t* src_v;   /* device: the visible image of slot b */
    const uint8_t* src_l;   /* device: the LWIR image of slot b */
    int32_t h, w;           /* source size */
    int32_t nh, nw;         /* resized content size */
    int32_t top, left;      /* where the content sits in the output */
    int32_t interp;         /* 0 = LINEAR, 1 = AREA */
    int32_t reserved;       /* 0 */
} DykResizePadRec;
typedef struct DykResizePadDesc {
    const DykResizePadRec* recs;        /* device [B] */
    const DykResizePadRec* recs_host;   /* host [B], the same records */
    uint8_t* dst_v;                     /* [B][3][Ho][Wo] */
    uint8_t* dst_l;                     /* [B][3][Ho][Wo] */
    int32_t B, Ho, Wo;
    int32_t layout;                     /* 0 = planar [3][h][w], 1 = interleaved [h][w][3] with the channels reversed */
    uint8_t color[3];                   /* border value per OUTPUT plane */
    uint8_t reserved[5];                /* 0 */
} DykResizePadDesc;
int dyk_resize_pad_pairs(const DykResizePadDesc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * Anchor clustering on the device (reference other_utils/anchor_cluster.py: wh_iou :153, k_means :169, anchor_fitness :199 and
 * the genetic loop of anchor_cluster :219): dyk_anchor_assign, dyk_anchor_median, dyk_anchor_fitness.  The host side
 * (other_utils/anchor_cluster.py) keeps the label readers, the random draws and the accept decisions; every N-sized pass is
 * made here.  What follows is this project's own rule; tests/anchor_ref.py restates it in numpy and the entries are held to
 * that restatement bit for bit.
 *
 * Common.  Boxes wh[N][2] = (w, h) and centres c[K][2] are contiguous, both fp32 (elem_bytes 4) or both fp64 (elem_bytes 8).
 * 1 <= K <= DYK_ANCHOR_MAX_K, 1 <= N <= DYK_ANCHOR_MAX_N (N < 2^27), 1 <= G <= DYK_ANCHOR_MAX_G.  Every box and every anchor is
 * finite and > 0.  Every floating-point operation below is rounded on its own: no fused multiply-add, no reassociation.
 *
 * dyk_anchor_assign : ONE launch (after a memset of stats).  In the type T of the inputs, per box i and centre k:
 *     inter = min(w, cw) * min(h, ch)
 *     iou   = inter / (((w * h) + (cw * ch)) - inter)
 *     d     = 1 - iou
 *     nearest[i] = the SMALLEST k that attains the minimum of d (np.argmin; ties that only the rounding of 1 - iou creates
 *                  count as ties)
 *   stats[0..K) = counts: the number of i with nearest[i] == k.  Exact.
 *   stats[K]    = changed: the number of i whose new nearest[i] differs from the value the buffer held before the launch.
 *   stats[K+1]  = bad: the number of rows i with w or h not finite or not > 0.  Such a row gets nearest[i] = 0 and is counted
 *                 in counts[0]; a caller that sees bad != 0 has no result.
 *   Integer atomics only (workgroup partials in LDS, one global integer add per workgroup and non-zero counter): every
 *   output is a pure function of the inputs.
 *
 * dyk_anchor_median : all 2K (cluster k, coordinate j) selections together.  The members of k are the i with
 *   nearest[i] == k, m of them.  x[0] <= ... <= x[m-1] their wh[i][j] in order:
 *     m odd  : c[k][j] = x[(m-1)/2]
 *     m even : c[k][j] = (x[m/2 - 1] + x[m/2]) / 2   in T (one add, one divide)
 *     m == 0 : c[k][j] is left as it was (a NAMED DEPARTURE from the reference, whose np.median of nothing is NaN)
 *   Selection is a radix select over the bit pattern (positive finite floats order as unsigned integers), 8 bits per pass
 *   from the top (4 passes in fp32, 8 in fp64).  A pass is a histogram launch over all boxes (256 integer bins per selection
 *   in LDS, 16 clusters per launch, added to the workspace with integer atomics) and a pick launch (one workgroup per
 *   selection takes the digit that holds the rank).  Where the upper middle is not the lower middle's value it is the
 *   smallest member above it (one more launch over the boxes, an integer minimum); a last launch writes the centres.  The
 *   kernel boundaries order these launches; nothing is handed over inside one.  Integer counts only: the result is a pure
 *   function of (wh, nearest).  Each coordinate on its own, as np.median(axis=0).  Values of nearest outside [0, K) belong to
 *   no cluster.  ws: dyk_anchor_median_ws_bytes(K) bytes, 8-byte aligned (0 for K out of range); its content is scratch.
 *
 * dyk_anchor_fitness : two launches (partials over (blocks of boxes) x G, then a fold); no atomics, no in-launch hand-off.
 *   Boxes fp32 or fp64, promoted exactly to fp64; candidates a[G][K][2] and thr in fp64.  Per candidate g, box i, anchor k,
 *   coordinate j, all in fp64:
 *     r = wh[i][j] / a[g][k][j];   q = 1.0 / r  (a second rounded division, NOT a / wh);   m = min(r, q)
 *     x[i][k] = min(m for j = 0, m for j = 1)
 *   "boxes"   : b[i] = max over k of x[i][k];  term[i] = b[i] if b[i] > thr else +0.0  (strict);
 *               fit_boxes[g] = S / (double)N,  hit_boxes[g] = the number of i with b[i] > thr,
 *     where S is the sum of term[i] in THIS ORDER.  Item p is the boxes [DYK_ANCHOR_FIT_ITEM * p, DYK_ANCHOR_FIT_ITEM * (p+1))
 *     below N; one workgroup of 256 threads per (item, g).  Thread t adds term[1024 p + t], [.. + t + 256], [.. + t + 512],
 *     [.. + t + 768] in that order to an accumulator that starts at +0.0 (a box at or past N adds +0.0).  The 64 lanes of a
 *     wave fold as l += l+32, l+16, l+8, l+4, l+2, l+1; the four waves add as ((w0 + w1) + w2) + w3: the item partial.  Fold:
 *     one wave per g; lane l adds the partials of items l, l + 64, l + 128, ... in that order to an accumulator that starts at
 *     +0.0, the lanes fold as above.  Every term is >= +0.0, so the zeros of absent boxes and items change no bit: S is a
 *     function of (wh, a[g], thr) only, identical from run to run and independent of G and of the grid.
 *   "anchors" : t[k] = max over i of x[i][k]  (exact in any order);
 *               fit_anchors[g] = (the sum over k = 0 .. K-1, in that order from +0.0, of t[k] if t[k] > thr else +0.0) / (double)K
 *               hit_anchors[g] = the number of k with t[k] > thr.  (What the reference's call anchor_fitness(k, wh, thr)
 *               computes, its arguments being swapped against the definition.)
 *   ws: dyk_anchor_fitness_ws_bytes(N, G, K) bytes, 8-byte aligned (0 for arguments out of range).
 *
 * DYK_ERR_ARG before any launch: a NULL descriptor or pointer, N, K, G out of range, elem_bytes not 4 or 8, a pointer not
 * aligned to its element (ws: 8 bytes), ws_bytes too small, thr not finite.  No kernel indexes past N, K or G.
 * ---------------------------------------------------------------------------------- */
#define DYK_ANCHOR_MAX_K 32
#define DYK_ANCHOR_MAX_N ((1 << 27) - 1)
#define DYK_ANCHOR_MAX_G 4096
#define DYK_ANCHOR_FIT_ITEM 1024
typedef struct DykAnchorAssignDesc {
    const void* wh;        /* device [N][2] */
    const void* c;         /* device [K][2] */
    int32_t* nearest;      /* device [N]: read (previous assignment), then written */
    int32_t* stats;        /* device [K + 2]: counts, changed, bad */
    int32_t N, K;
    int32_t elem_bytes;    /* 4 = fp32, 8 = fp64 */
    int32_t reserved;      /* 0 */
} DykAnchorAssignDesc;
typedef struct DykAnchorMedianDesc {
    const void* wh;            /* device [N][2] */
    const int32_t* nearest;    /* device [N] */
    void* c;                   /* device [K][2]: written except for empty clusters */
    void* ws;                  /* device, dyk_anchor_median_ws_bytes(K) bytes */
    int64_t ws_bytes;
    int32_t N, K;
    int32_t elem_bytes;
    int32_t reserved;
} DykAnchorMedianDesc;
typedef struct DykAnchorFitnessDesc {
    const void* wh;            /* device [N][2] */
    const double* a;           /* device [G][K][2] */
    void* ws;                  /* device, dyk_anchor_fitness_ws_bytes(N, G, K) bytes */
    double* fit_boxes;         /* device [G] */
    double* fit_anchors;       /* device [G] */
    int32_t* hit_boxes;        /* device [G] */
    int32_t* hit_anchors;      /* device [G] */
    int64_t ws_bytes;
    double thr;
    int32_t N, K, G;
    int32_t elem_bytes;        /* of wh */
} DykAnchorFitnessDesc;
int dyk_anchor_assign(const DykAnchorAssignDesc* desc, void* stream);
int64_t dyk_anchor_median_ws_bytes(int32_t K);
int dyk_anchor_median(const DykAnchorMedianDesc* desc, void* stream);
int64_t dyk_anchor_fitness_ws_bytes(int32_t N, int32_t G, int32_t K);
int dyk_anchor_fitness(const DykAnchorFitnessDesc* desc, void* stream);

/* Profiling variant of dyk_run_commands: brackets every command with HIP events on `stream`
 * and, after synchronising the stream, writes each command's duration in milliseconds to
 * ms_out[0..n).  Used by bench.py's roofline pass, never in a timed throughput region. */
int dyk_run_commands_timed(const DykCommand* cmds, int32_t n, void* stream, float* ms_out_host);
/* The same for the entries of a schedule, in issue order on ONE stream (two-problem entries as the single launch they
 * are in the step): ms_out[k] = duration of entry k. */
int dyk_run_schedule_timed(const DykCommand* cmds, const DykSchedEntry* sched, int32_t n_entries, void* stream,
                           float* ms_out_host);
/* Library stream idx (1..7) of the current device's schedule runtime (the streams dyk_run_schedule replays on; created on
 * first use).  For host code with side-stream work of its own: the HIP runtime maps all streams of a process onto four
 * hardware queues, so such work goes onto one of these rather than onto a fifth stream. */
int dyk_sched_stream(int32_t idx, void** stream_out);

#ifdef __cplusplus
}
#endif
#endif /* DYK_HIP_H */
