// C-ABI front end of the implicit-GEMM convolution: argument validation and the choice of the pixel-tile
// instantiation (conv_igemm_n{80,128,160}.hip; kernel in conv_igemm_kernel.h).
#include <stddef.h>
#include <string.h>
#include "conv_tune.h"

static int conv_validate(const DykConvDesc* d) {
    if (!d || !d->x || !d->w || !d->y) return DYK_ERR_ARG;
    if (d->ntaps < 0 || d->ntaps > DYK_MAX_TAPS) return DYK_ERR_ARG;
    if (d->B <= 0 || d->Hg <= 0 || d->Wg <= 0 || d->Cout <= 0 || d->Cin <= 0) return DYK_ERR_ARG;
    if (d->ncls < 0 || d->ncls > 4) return DYK_ERR_ARG;
    for (int c = 0; c < (d->ncls > 1 ? d->ncls : 0); ++c)
        if (d->cls_first[c] < 0 || d->cls_ntaps[c] < 0 || d->cls_first[c] + d->cls_ntaps[c] > d->ntaps || d->cls_ooy[c] < 0 ||
            d->cls_ooy[c] >= d->osy || d->cls_oox[c] < 0 || d->cls_oox[c] >= d->osx)
            return DYK_ERR_ARG;
    // f16 is the inference type: forward epilogues only (no statistics, no fused BatchNorm forms)
    if (d->dtype == DYK_F16 && (d->flags & (DYK_EPI_STATS | DYK_EPI_BNFWD | DYK_EPI_BNBWD | DYK_EPI_ADDEND))) return DYK_ERR_UNSUPPORTED;
    if ((d->flags & DYK_EPI_STATS) && !d->stats) return DYK_ERR_ARG;
    if ((d->flags & DYK_EPI_RESIDUAL) && !d->res) return DYK_ERR_ARG;
    if ((d->flags & DYK_EPI_ADDEND) && (!(d->flags & DYK_EPI_BNBWD) || ((uintptr_t)d->add % 16))) return DYK_ERR_ARG;     // (add == NULL: zero addend)
    if (d->flags & DYK_EPI_BNFWD) {
        // conv + BatchNorm + activation in one launch: statistics on, bf16, one problem, whole 16-byte channel chunks
        if (!(d->flags & DYK_EPI_STATS) || (d->flags & (DYK_EPI_AFFINE | DYK_EPI_ACCUM | DYK_EPI_OUT_F32 | DYK_EPI_BNBWD | DYK_EPI_ADDEND)))
            return DYK_ERR_ARG;
        if (d->dtype != DYK_BF16 || d->twin || d->ncls > 1 || d->bn_count <= 0) return DYK_ERR_ARG;
        if (!d->y2 || !d->bn_counter || !d->scale || !d->shift || ((uintptr_t)d->y2 % 16) || ((uintptr_t)d->bn_counter % 8)) return DYK_ERR_ARG;
        if (d->Cout % 8 || d->ldy % 8 || d->ldy2 % 8 || d->ldy2 < d->Cout) return DYK_ERR_ARG;
        if ((d->flags & DYK_EPI_RESIDUAL) && (d->ldr % 4 || ((uintptr_t)d->res % 8))) return DYK_ERR_ARG;
        if ((long)d->B * d->Ho * d->Wo * d->ldy2 >= (1L << 31)) return DYK_ERR_ARG;
    }
    if (d->flags & DYK_EPI_BNBWD) {
        if (d->flags & (DYK_EPI_AFFINE | DYK_EPI_RESIDUAL | DYK_EPI_STATS | DYK_EPI_ACCUM | DYK_EPI_OUT_F32)) return DYK_ERR_ARG;
        if (!d->res || !d->stats || !d->scale || !d->shift || !d->aux0 || !d->aux1) return DYK_ERR_ARG;
        const int es = d->dtype == DYK_F32 ? 4 : 2;
        // needs the staged (vector) epilogue: 16-byte aligned rows of y and res, whole 16-byte channel chunks
        if (d->Cout % (16 / es) || ((size_t)d->ldy * es) % 16 || ((size_t)d->ldr * es) % 16 || ((uintptr_t)d->y % 16) ||
            ((uintptr_t)d->res % 16))
            return DYK_ERR_ARG;
    }
    if (d->splitk > 1) {
        // split-K across workgroups: private scratch + zeroed counters; one problem, one parity class, no in-launch BatchNorm
        if (d->splitk > 16 || !d->sk_ws || !d->sk_cnt || ((uintptr_t)d->sk_ws % 16) || ((uintptr_t)d->sk_cnt % 4) || d->sk_cnt_n <= 0 ||
            d->sk_ws_bytes <= 0)
            return DYK_ERR_ARG;
        if (d->twin || d->ncls > 1 || (d->flags & DYK_EPI_BNFWD)) return DYK_ERR_ARG;
    }
    if (d->dtype != DYK_BF16 && d->dtype != DYK_F32 && d->dtype != DYK_F16) return DYK_ERR_ARG;
    const int epv = d->dtype == DYK_F32 ? 4 : 8;
    if (d->ldx % epv || ((uintptr_t)d->x % 16) || ((uintptr_t)d->w % 16)) return DYK_ERR_ARG;
    // 32-bit element offsets inside the kernel
    if ((long)d->B * d->Hi * d->Wi * d->ldx >= (1L << 31)) return DYK_ERR_ARG;
    if ((long)d->B * d->Ho * d->Wo * d->ldy >= (1L << 31)) return DYK_ERR_ARG;
    if (d->Hi > 16000 || d->Wi > 16000) return DYK_ERR_ARG;
    return DYK_OK;
}

// validate, route (conv_tune.h), try the family; a family that refuses the problem hands it to its generic tile
extern "C" int dyk_conv_igemm(const DykConvDesc* d, void* stream) {
    int rc0 = conv_validate(d);
    if (rc0 != DYK_OK) return rc0;
    if (d->twin) {
        // two-problem launch: the twin must be a valid problem of its own and agree in every non-pointer field
        if ((rc0 = conv_validate(d->twin)) != DYK_OK) return rc0;
        const size_t lo = offsetof(DykConvDesc, dtype), hi = offsetof(DykConvDesc, twin);
        if (memcmp((const char*)d + lo, (const char*)d->twin + lo, hi - lo) != 0) return DYK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](int family) {
        switch (family) {
        case CONV_N80: return dyk_conv_launch_n80(d, s);
        case CONV_N160: return dyk_conv_launch_n160(d, s);
        case CONV_HALO4: return dyk_conv_launch_halo(d, s, 4);
        case CONV_HALO8: return dyk_conv_launch_halo(d, s, 8);
        case CONV_LT: return dyk_conv_launch_lt(d, s);
        // (resident-weight data gradient: bf16 without split-K only)
        case CONV_SC: return (d->splitk > 1 || d->dtype != DYK_BF16) ? (int)DYK_ERR_UNSUPPORTED : dyk_conv_launch_sc(d, s);
        case CONV_PW: return dyk_conv_launch_pw(d, s);
        case CONV_KG: return dyk_conv_launch_kg(d, s);
        default: return dyk_conv_launch_n128(d, s);
        }
    };
    const ConvRoute r = conv_route(d);
    const int rc = r.family < 0 ? r.family : launch(r.family);
    return (rc != DYK_ERR_UNSUPPORTED || r.fallback < 0 || conv_tune_nofallback(d->tune)) ? rc : launch(r.fallback);
}

extern "C" int dyk_conv_route(const DykConvDesc* d, int32_t* fallback_tile) {
    const ConvRoute r = d ? conv_route(d) : ConvRoute{DYK_ERR_ARG, -1};
    if (fallback_tile) *fallback_tile = r.fallback;
    return r.family;
}

extern "C" int dyk_conv_bnfwd_max_grid(void) { return 256; }

// workgroups of the generic-tile launch of `d`: of the tile DYK_EPI_BNFWD runs for its tune word, whatever the flags of `d`
// (halo / K-grouped / large-tile launches differ)
extern "C" int dyk_conv_grid(const DykConvDesc* d) {
    if (!d || d->B <= 0 || d->Hg <= 0 || d->Wg <= 0 || d->Cout <= 0) return DYK_ERR_ARG;
    const ConvTile t = conv_generic_tile(d, conv_route_bnfwd(d), false);
    const long n = (long)d->B * d->Hg * d->Wg;
    return (int)((n + t.bn - 1) / t.bn) * ((d->Cout + t.bm - 1) / t.bm) * (d->ncls > 1 ? d->ncls : 1);
}

// split-K scratch: bytes of sk_ws and words of sk_cnt that hold for every kernel the route of `d` can run (the family AND the
// generic tile it falls back to): S * 4 bytes * (Cout rounded up to the channel tile) * (positions rounded up to the pixel
// tile), tiles = their product counted in tiles
extern "C" int64_t dyk_conv_splitk_ws_bytes(const DykConvDesc* d, int32_t* tiles) {
    if (tiles) *tiles = 0;
    if (!d || d->B <= 0 || d->Hg <= 0 || d->Wg <= 0 || d->Cout <= 0) return DYK_ERR_ARG;
    if (d->splitk <= 1) return 0;
    // (DYK_EPI_BNFWD excludes split-K, conv_validate: under that flag the route is the generic one and the answer is moot)
    ConvRoute r = conv_route(d);
    if (r.family < 0) r = conv_route_bnfwd(d);                            // (a word no kernel runs: its generic tile)
    const long n = (long)d->B * d->Hg * d->Wg;
    int64_t bytes = 0;
    int32_t nt = 0;
    auto cover = [&](ConvTile t) {
        const int64_t tm = (d->Cout + t.bm - 1) / t.bm, tn = (n + t.bn - 1) / t.bn;
        const int64_t b = tm * tn * (int64_t)d->splitk * t.bm * t.bn * 4;
        if (b > bytes) bytes = b;
        if (tm * tn > nt) nt = (int32_t)(tm * tn);
    };
    // the generic tile as the word's channel code reads; under the K-grouped bit at least 64 rows, whichever kernel takes it.
    // (K-grouped with channel code 1 and Cout > 64 launches 128 rows, which this does not cover: launch_conv_impl refuses it)
    ConvTile g = conv_generic_tile(d, r, false);
    if (conv_tune_kgrouped(d->tune) && g.bm < 64) g.bm = 64;
    cover(g);
    if (r.family == CONV_LT) {
        const int shape = conv_tune_lt_shape(d->tune);
        cover(shape == 1 ? ConvTile{128, 320} : (shape == 2 ? ConvTile{256, 160} : ConvTile{128, 160}));
    }
    if (tiles) *tiles = nt;
    return bytes;
}
