// Shared pieces of the weight-gradient kernels (conv_wgrad.hip, conv_wgrad_rb.hip, conv_wgrad_ps.hip): the fields of the tune
// word, the K-split planner, the pixel-major LDS tile with its XOR chunk swizzle, the LDS-DMA wave instruction, SGPR-pinned
// pointers, the transposing fragment read, the grouped-launch prologue.  Each translation unit gets its own zero page.
#pragma once
#include "dyk_common.h"

namespace {

// ---- fields of DykWgradDesc.tune.  The layout is persisted (bench_tuning.json, users' tune caches): it does not change.
// bits 28..30: the kernel asked for -- 0 per-tap, 1 multi-tap 3x3, 2 row-block 3x3 (conv_wgrad_rb.hip), 3 pixel-streaming
// 1x1 (conv_wgrad_ps.hip); a variant the problem is not eligible for falls back to 0
constexpr int wg_tune_variant(int tune) { return (tune >> 28) & 7; }
// low byte = LDS ring stages (per-tap kernel: 2 | 3; pixel-streaming kernel: 0 = default, up to 8)
constexpr int wg_tune_stages(int tune) { return tune & 0xff; }
// bits 8..15 = K-groups per workgroup (per-tap kernel: 1 | 2; row-block kernel: 2 selects 256-pixel K steps)
constexpr int wg_tune_kgroups(int tune) { return (tune >> 8) & 0xff; }
// bits 24..27 = 1: tiles capped at 64 x 64 (small GEMMs: more tiles, so fewer K splits -- partial planes -- fill the chip)
constexpr bool wg_tune_cap64(int tune) { return ((tune >> 24) & 0xf) == 1; }
// pixel-streaming kernel: bits 8..11 tile cap (1 = 64 x 64), bits 12..15 pixels per stage (0 = by tile, 1 = 64, 2 = 128)
constexpr bool ps_tune_cap64(int tune) { return ((tune >> 8) & 0xf) == 1; }
constexpr int ps_tune_stage_len(int tune) { return (tune >> 12) & 0xf; }
// bit 20: the caller vouches that nobody else adds to dw while this launch runs (row-block and pixel-streaming kernels)
constexpr bool wg_tune_exclusive(int tune) { return (tune >> 20) & 1; }
// bits 16.. of `tune`: ablation switches for kernel analysis (tools/gpu_probe.py wgablate), never set by the plan
constexpr bool wg_tune_abl_noatomic(int tune) { return (tune >> 16) & 1; }
constexpr bool wg_tune_abl_noloop(int tune) { return (tune >> 17) & 1; }

// ---- K-split plan of a launch: `steps` K steps over `tiles` output tiles.  requested <= 0: as many splits as bring the launch
// to `target` workgroups, every K-group keeping at least `min_steps` steps.  Returns the split count and the steps per
// workgroup (a multiple of `kgroups`; 1 where the kernel has none).  literal: a plane / fold mode with a given count writes
// exactly that many planes (trailing empty ones with zeros); otherwise splits that would own no step are dropped.  Both
// numbers decide the summation order, hence the bits of the result.
struct WgSplitPlan {
    int splits, chunk;
};
inline WgSplitPlan wg_plan_splits(int steps, int tiles, int target, int min_steps, int kgroups, int requested, bool literal) {
    int splits = requested;
    if (splits <= 0) {
        splits = dyk_div_up(target, tiles);
        const int max_splits = steps / (min_steps * kgroups) > 0 ? steps / (min_steps * kgroups) : 1;
        if (splits > max_splits) splits = max_splits;
    }
    if (splits * kgroups > steps) splits = steps / kgroups > 0 ? steps / kgroups : 1;
    const int chunk = dyk_div_up(steps, splits * kgroups) * kgroups;
    if (!literal) splits = dyk_div_up(steps, chunk);
    return {splits, chunk};
}

// the standard 3x3 / pad 1 tap table (tdy = t/3 - 1, tdx = t%3 - 1) the multi-tap and row-block kernels are written for
inline bool wg_std3x3_taps(const DykWgradDesc* d) {
    if (d->ntaps != 9) return false;
    for (int t = 0; t < 9; ++t)
        if (d->tdy[t] != t / 3 - 1 || d->tdx[t] != t % 3 - 1) return false;
    return true;
}

// a wave-uniform pointer pinned in SGPRs (the compiler cannot re-materialise it by re-loading the kernel argument in the loop)
template <typename P> __device__ inline P* wg_sgpr_ptr(P* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (P*)(((unsigned long long)hi << 32) | lo);
}

typedef short v4i16_t __attribute__((__vector_size__(4 * sizeof(short))));
#define LDS_AS __attribute__((address_space(3)))

// byte offset of (row, channel) in a [ROWS][C] tile, row bytes RB = C*sizeof(T)
template <typename T, int C> __device__ inline int wg_off(int row, int ch) {
    constexpr int RB = C * (int)sizeof(T);
    if (sizeof(T) == 2) {
        constexpr int NCH = RB / 32;                     // 32-byte chunks per row
        // A 32-lane group of the transposing fragment read touches ONE 32-byte chunk column of the eight rows
        // b + {0,1,2,3, 8,9,10,11} (b = K offset of the step, plus the tap shift in the multi-tap kernel: any value).  Rows
        // that are congruent modulo 256 / RB share their banks, so the XOR key must tell exactly those rows apart -- from row
        // bits that differ for ANY b: 256-byte rows (all eight collide) bits 0,1,3; 128-byte rows (the four of equal parity
        // collide) bits 1,3; 64-byte rows (b + i and b + 8 + i collide) bit 3.  (Rounds 1-3 keyed every width with
        // `row & 3 | bit 3 << 2` masked to the chunk count: right for 256-byte rows only -- 64-wide tiles, i.e. every dy tile
        // of the multi-tap kernel, read with 2-way conflicts: 57 % of its LDS cycles in the round-3 counters.)
        const int f = NCH >= 8 ? ((row & 3) | (((row >> 3) & 1) << 2)) & (NCH - 1)
                    : NCH == 4 ? (((row >> 1) & 1) | (((row >> 3) & 1) << 1))
                    : NCH == 2 ? ((row >> 3) & 1) : 0;
        const int chunk = (ch >> 4) ^ f;
        return row * RB + chunk * 32 + (ch & 15) * 2;
    } else {
        constexpr int NCH = RB / 64;                     // 64-byte chunks per row
        const int chunk = (ch >> 4) ^ (row & 1 & (NCH - 1));
        return row * RB + chunk * 64 + (ch & 15) * 4;
    }
}

// one LDS-DMA wave instruction (see conv_igemm.hip: issued via inline asm so that hipcc does not
// drain vmcnt(0) in front of every LDS read while the ring is in flight)
static __device__ uint4 dyk_wg_zero_page[8];
__device__ inline void wg_glds16(const void* gsrc, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_addr)
                 : "memory");
}
__device__ inline unsigned wg_lds_addr(const void* p) {
    return __builtin_amdgcn_readfirstlane((unsigned)(size_t)(LDS_AS const char*)p);
}

// transposing fragment read (ds_read_b64_tr_b16, see conv_wgrad.hip): the eight bf16 of a lane's MFMA operand, four K
// pixels from each of the two addresses
__device__ __forceinline__ uint2 wg_tr_read4(const char* p) {
    return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS v4i16_t*)(LDS_AS char*)p));
}
__device__ __forceinline__ uint4 wg_tr_read(const char* p0, const char* p1) {
    const uint2 lo = wg_tr_read4(p0), hi = wg_tr_read4(p1);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// grouped launch (DykWgradDesc.group): problem p owns blocks [p per, (p + 1) per); its tensors come out of the device table
// (scalar loads).  Returns the entry of the block's problem; `bid` becomes the block id inside that problem.  (The caller
// keeps the `group_n > 0` test and copies the four pointers itself: with them inside the helper the row-block kernel compiles
// to other instructions.)
__device__ __forceinline__ const DykWgradGroupEntry* wg_group_select(const DykWgradGroupEntry* group, int tiles_m, int tiles_n,
                                                                     int splits, int& bid) {
    const int per = tiles_m * tiles_n * splits;
    const int prob = __builtin_amdgcn_readfirstlane(bid / per);
    bid -= prob * per;
    return wg_sgpr_ptr(group) + prob;
}

// logical channel stored at physical 16-byte slot `ps` of tile row `row` (inverse of wg_off's swizzle,
// which is an XOR on the 32-byte (bf16) / 64-byte (f32) chunk index and therefore its own inverse)
template <typename T, int C> __device__ inline int wg_logical_ch(int row, int ps) {
    constexpr int EPV = 16 / (int)sizeof(T);
    return (wg_off<T, C>(row, ps * EPV) - row * C * (int)sizeof(T)) / (int)sizeof(T);
}

}  // namespace
