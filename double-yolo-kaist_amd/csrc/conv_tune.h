// Front end of the forward / data-gradient convolution (dyk_conv_igemm): the fields of DykConvDesc.tune, the tile of the
// generic kernels, the route of a descriptor (kernel family + generic fallback) and the per-translation-unit entry points.
#pragma once
#include "dyk_common.h"

// ---- DykConvDesc.tune.  The layout is persisted (bench_tuning.json, users' tune caches): it does not change.
//   shared by every family
//     bits  0..7   K-step bytes: 64 | 128, 0 = the kernel's default (a 128 that the row length does not allow is ignored)
//     bits 12..15  pixel-tile code = the kernel family asked for: 0 generic 128 pixels, 1 generic 80, 2 generic 160, 3 / 4 halo
//                  kernel with 4x20 / 8x20 patches, 5 large-tile 3x3 (conv_lt_kernel.h), 6 resident-weight 3x3 data gradient
//                  (conv_sc.hip), 7 persistent pointwise (conv_pw_kernel.h); 8..15 read as 0.  fp32 has the 128-pixel tile only:
//                  every code reads as 0
//     bits 16..22  ablation switches for kernel analysis (tools/gpu_probe.py ablate), never set by the plan
//     bit  23      analysis: no fallback -- a family that refuses the problem returns DYK_ERR_UNSUPPORTED
//     bits 28..30  1 = K-grouped workgroups (two 4-wave groups over the halves of Cin): codes 1 / 2, tried before the halo codes
//   per pixel-tile code
//     bits  8..11  codes 0..4: LDS ring stages (2 | 3 | 4 | 6, else 2; halo and K-grouped kernels: fixed);
//                  code 5: shape (1 = 128 x 320, 2 = 256 x 160, 3 = 128 x 160 with two K-groups); code 7: ring stages `nxs` (0 = 3)
//     bits 24..27  codes 0..4, 6: channel-tile code (0 = by Cout, 1 = 32, 2 = 64, 3 = 128 rows);
//                  code 5: patch-width code (0 = fewest halo rows, k: 10 << k pixels);
//                  code 7: bit 24 = 128-pixel tiles (`bn128`), bit 25 = 32-pixel tiles (`bn32`)
//   Aliasing: a family that refuses a problem hands it to a GENERIC tile, which reads the same word under the generic meaning.
//     code 5 -> 160-pixel tile: ring stages = the shape (3 stays 3, 1 / 2 read as 2); bits 24..27 are NOT read as a channel tile
//               (conv_chan_code: the channel tile goes by Cout) -- except under DYK_EPI_BNFWD, which never runs family 5
//     code 7 -> 128-pixel tile: ring stages = nxs; bn128 reads as channel code 1 (32 rows), bn32 as channel code 2 (64 rows),
//               whatever Cout is
constexpr int conv_tune_kstep(int tune) { return tune & 0xff; }
constexpr int conv_tune_stages(int tune) { return (tune >> 8) & 0xf; }
constexpr int conv_tune_lt_shape(int tune) { return (tune >> 8) & 0xf; }
constexpr int conv_tune_lt_patch(int tune) { return (tune >> 24) & 0xf; }
constexpr int conv_tune_pw_nxs(int tune) { return (tune >> 8) & 0xf; }
constexpr bool conv_tune_pw_bn128(int tune) { return (tune >> 24) & 1; }
constexpr bool conv_tune_pw_bn32(int tune) { return (tune >> 25) & 1; }
constexpr bool conv_tune_kgrouped(int tune) { return ((tune >> 28) & 7) == 1; }
constexpr bool conv_tune_nofallback(int tune) { return (tune >> 23) & 1; }
// ablation bits (as int: with a bool accessor conv_lt_kernel allocates other registers): no output stores / no K loop / empty
// kernel / tables only / no epilogue (the accumulators stay alive) / no batched split-K fold / K loop without its workgroup
// barrier (WRONG results: timing only)
constexpr int conv_tune_abl_nostore(int tune) { return (tune >> 16) & 1; }
constexpr int conv_tune_abl_noloop(int tune) { return (tune >> 17) & 1; }
constexpr int conv_tune_abl_empty(int tune) { return (tune >> 18) & 1; }
constexpr int conv_tune_abl_tables(int tune) { return (tune >> 19) & 1; }
constexpr int conv_tune_abl_noepi(int tune) { return (tune >> 20) & 1; }
constexpr int conv_tune_abl_nofold(int tune) { return (tune >> 21) & 1; }
constexpr int conv_tune_abl_nobar(int tune) { return (tune >> 22) & 1; }

// pixel-tile codes = kernel families (dyk_conv_route returns these); the first three are the generic tiles
enum { CONV_N128 = 0, CONV_N80 = 1, CONV_N160 = 2, CONV_HALO4 = 3, CONV_HALO8 = 4, CONV_LT = 5, CONV_SC = 6, CONV_PW = 7, CONV_KG = 8 };
inline int conv_tile_code(const DykConvDesc* d) { return d->dtype != DYK_F32 ? (d->tune >> 12) & 0xf : CONV_N128; }
// the generic tile of a pixel-tile code
constexpr int conv_generic_of(int tile) {
    return (tile == CONV_N80 || tile == CONV_HALO4) ? CONV_N80 : ((tile == CONV_N160 || tile == CONV_HALO8) ? CONV_N160 : CONV_N128);
}

// ---- route of a descriptor: the family dyk_conv_igemm tries first and the generic tile that takes the problem when the family
// refuses it (-1: none -- the generic families refuse nothing they could hand on).  family < 0: an error code, nothing runs.
struct ConvRoute { int family, fallback; };
// under DYK_EPI_BNFWD: generic tiles only carry this epilogue (also what dyk_conv_grid counts, whatever the flags)
inline ConvRoute conv_route_bnfwd(const DykConvDesc* d) { return {conv_generic_of(conv_tile_code(d)), -1}; }
inline ConvRoute conv_route(const DykConvDesc* d) {
    const int tile = conv_tile_code(d);
    if (d->flags & DYK_EPI_BNFWD) return conv_route_bnfwd(d);
    if (tile == CONV_LT) return {CONV_LT, CONV_N160};
    if (tile == CONV_SC || tile == CONV_PW) return {tile, CONV_N128};     // (family 6 also refuses split-K and f16: dyk_conv_igemm)
    if (conv_tune_kgrouped(d->tune)) {
        if (tile == CONV_N80 || tile == CONV_N160) return {CONV_KG, tile};
        // a tile code the K-grouped kernels do not build means what it means without the bit -- unless the word forbids fallbacks
        if (conv_tune_nofallback(d->tune)) return {DYK_ERR_UNSUPPORTED, -1};
    }
    if (tile == CONV_HALO4 || tile == CONV_HALO8) return {tile, conv_generic_of(tile)};
    return conv_route_bnfwd(d);
}

// bits 24..27 as a channel-tile code under route `r`: family 5 keeps its patch width there
inline int conv_chan_code(const DykConvDesc* d, ConvRoute r) { return r.family == CONV_LT ? 0 : (d->tune >> 24) & 0xf; }

// ---- channel x pixel tile of the generic kernel that runs `d` under route `r` (the family itself or its fallback), the one
// place these rules live.  min64: kernels without a 32-row form (K-grouped, halo), which do not read channel code 1 either
struct ConvTile { int bm, bn; };
inline ConvTile conv_generic_tile(const DykConvDesc* d, ConvRoute r, bool min64) {
    const int tile = r.fallback >= 0 ? r.fallback : r.family;
    const int bn = tile == CONV_N80 ? 80 : (tile == CONV_N160 ? 160 : 128);
    int bm = d->Cout > 64 ? 128 : (d->Cout > 32 ? 64 : 32);
    const int code = conv_chan_code(d, r);
    if (code >= (min64 ? 2 : 1) && code <= 3) bm = 16 << code;
    if ((bn == 80 || min64) && bm == 32) bm = 64;                         // an 80-pixel tile: a wave needs 16 channel rows
    return {bm, bn};
}

// ---- entry points of the translation units (one per family, element type and epilogue family, so that make -j builds them in
// parallel); DYK_ERR_UNSUPPORTED = not this unit's problem
typedef int ConvLaunchFn(const DykConvDesc* d, hipStream_t s);
typedef int ConvHaloLaunchFn(const DykConvDesc* d, hipStream_t s, int th);
ConvLaunchFn dyk_conv_launch_n128, dyk_conv_launch_n128b, dyk_conv_launch_n128f, dyk_conv_launch_n128n, dyk_conv_launch_n128h;
ConvLaunchFn dyk_conv_launch_n80, dyk_conv_launch_n80b, dyk_conv_launch_n80n, dyk_conv_launch_n80h;
ConvLaunchFn dyk_conv_launch_n160, dyk_conv_launch_n160b, dyk_conv_launch_n160n, dyk_conv_launch_n160h;
ConvHaloLaunchFn dyk_conv_launch_halo, dyk_conv_launch_halob, dyk_conv_launch_haloh;
ConvLaunchFn dyk_conv_launch_kg, dyk_conv_launch_kgh, dyk_conv_launch_lt, dyk_conv_launch_ltb, dyk_conv_launch_lth;
ConvLaunchFn dyk_conv_launch_sc, dyk_conv_launch_pw, dyk_conv_launch_pwb, dyk_conv_launch_pwc, dyk_conv_launch_pwh;
