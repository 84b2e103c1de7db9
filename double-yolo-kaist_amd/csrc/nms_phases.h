// Phases 2 to 4 of the NMS launch -- sort, greedy suppression, merge -- in one definition, shared by nms_kernel (nms.hip: one
// thread per (row, class) pair builds the candidates) and nms_rows_kernel (nms_rows.hip: a wavefront per alive row does).
// Both hand over the same thing: cand[0..n) in (row, class) order, keys[o] = (inverted score bits << 32) | o, n
// workgroup-uniform and > 0, keys[] with room for n rounded up to a power of two.  See nms.hip for what each phase restates.
#pragma once
#include "dyk_common.h"

#pragma clang fp contract(off)

namespace nmsp {

constexpr int NT = 1024;
constexpr int MAX_KEEP = 512;
constexpr int MB = 4;          // kept boxes one wavefront merges per pass over the candidates

struct Cand {
    float x1, y1, x2, y2, conf, cls;
    int row;
};

// the kept list of phase 3 (LDS), read again by phase 4
struct Kept {
    float x1[MAX_KEEP], y1[MAX_KEEP], x2[MAX_KEEP], y2[MAX_KEEP], ar[MAX_KEEP];
    int n;
};

// keys + candidates of one image holding up to `cap` candidates, rounded up to 256 bytes
__host__ __device__ inline long ws_bytes(long cap) {
    long P = 1;
    while (P < cap) P <<= 1;
    const long bytes = P * 8 + cap * (long)sizeof(Cand);
    return (bytes + 255) / 256 * 256;
}

__device__ inline unsigned long long sort_key(float conf, int o) {
    const unsigned int sb = __float_as_uint(conf);                            // conf > 0: bits are monotonic
    return ((unsigned long long)(0xFFFFFFFFu - sb) << 32) | (unsigned int)o;
}

__device__ inline float iou_tv(float ax1, float ay1, float ax2, float ay2, float aarea, float bx1, float by1, float bx2,
                               float by2, float barea) {
    const float xx1 = fmaxf(ax1, bx1), yy1 = fmaxf(ay1, by1);
    const float xx2 = fminf(ax2, bx2), yy2 = fminf(ay2, by2);
    const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
    const float inter = w * h;
    return inter / ((aarea + barea) - inter);
}

// MERGE = false is the plain kernel: every merge statement sits under `if constexpr (MERGE)`.  D is DykNmsDesc or
// DykNmsRowsDesc (the fields read here mean the same in both).  Called by all NT threads of image b's workgroup; the
// candidate stores of the caller need no barrier of their own, the one behind the key padding orders them too.
template <bool MERGE, class D>
__device__ inline void sort_suppress_merge(const D& d, unsigned long long* keys, const Cand* cand, const int n, Kept& kept) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // ---------------------------------------------------------------- 2. sort (bitonic, padded to a power of two)
    long Pn = 1;
    while (Pn < n) Pn <<= 1;
    for (long i = n + tid; i < Pn; i += NT) keys[i] = ~0ull;
    __syncthreads();
    for (long k = 2; k <= Pn; k <<= 1) {
        for (long j = k >> 1; j > 0; j >>= 1) {
            for (long i = tid; i < Pn; i += NT) {
                const long ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = keys[i], bb = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > bb) == up) { keys[i] = bb; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
    // ---------------------------------------------------------------- 3. greedy suppression (wave 0)
    const int max_keep = d.max_num < MAX_KEEP ? d.max_num : MAX_KEEP;
    if (wv == 0) {
        int nkept = 0;
        const float off_mul = d.agnostic ? 0.f : 4096.f;                       // :446-447 class offset
        for (int start = 0; start < n && nkept < max_keep; start += 64) {
            const int i = start + lane;
            bool alive = i < n;
            int ci = 0;
            float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, area = 0.f;
            if (alive) {
                ci = (int)(keys[i] & 0xFFFFFFFFu);
                const Cand c = cand[ci];
                const float o = c.cls * off_mul;
                x1 = c.x1 + o; y1 = c.y1 + o; x2 = c.x2 + o; y2 = c.y2 + o;
                area = (x2 - x1) * (y2 - y1);
                for (int k = 0; k < nkept && alive; ++k)
                    if (iou_tv(kept.x1[k], kept.y1[k], kept.x2[k], kept.y2[k], kept.ar[k], x1, y1, x2, y2, area) > d.iou_thres) alive = false;
            }
            for (int s = 0; s < 64 && nkept < max_keep; ++s) {
                const bool sa = __shfl((int)alive, s, 64) != 0;
                if (!sa) continue;
                const float sx1 = __shfl(x1, s, 64), sy1 = __shfl(y1, s, 64), sx2 = __shfl(x2, s, 64), sy2 = __shfl(y2, s, 64);
                const float sar = __shfl(area, s, 64);
                if (lane == s) {
                    kept.x1[nkept] = x1; kept.y1[nkept] = y1; kept.x2[nkept] = x2; kept.y2[nkept] = y2; kept.ar[nkept] = area;
                    const Cand c = cand[ci];
                    float* o = d.out + ((long)b * d.max_num + nkept) * 6;
                    o[0] = c.x1; o[1] = c.y1; o[2] = c.x2; o[3] = c.y2; o[4] = c.conf; o[5] = c.cls;
                    d.out_rows[(long)b * d.max_num + nkept] = c.row;
                }
                if (lane > s && alive && iou_tv(sx1, sy1, sx2, sy2, sar, x1, y1, x2, y2, area) > d.iou_thres) alive = false;
                ++nkept;
            }
            __builtin_amdgcn_wave_barrier();       // kept-list LDS writes precede the next chunk's reads
        }
        if (lane == 0) {
            d.counts[b] = nkept;
            if constexpr (MERGE) kept.n = nkept;
        }
    }
    // ---------------------------------------------------------------- 4. merge (all 16 wavefronts)
    if constexpr (MERGE) {
        __syncthreads();                           // kept list, kept.n and wave 0's out[] rows are complete (n is uniform)
        if (n > 1 && n < 3000) {                   // :450, both strict; n counts candidates, not rows
            const int nkept = kept.n;
            const float off_mul = d.agnostic ? 0.f : 4096.f;
            // MB kept boxes per pass over the candidates: the loop is bound by the latency of the cand[] load, which the
            // MB boxes share (measured, 16 x (n = 2999, 100 kept): 105 us with one box per pass, 76 us with four)
            for (int base = wv * MB; base < nkept; base += (NT / 64) * MB) {
                float bx1[MB], by1[MB], bx2[MB], by2[MB], bar[MB];                                  // boxes[i[k]], offset
                double acc[MB][5];
#pragma unroll
                for (int q = 0; q < MB; ++q) {
                    const int k = min(base + q, nkept - 1);                                         // (past the end: recomputed, not written)
                    bx1[q] = kept.x1[k]; by1[q] = kept.y1[k]; bx2[q] = kept.x2[k]; by2[q] = kept.y2[k]; bar[q] = kept.ar[k];
#pragma unroll
                    for (int c = 0; c < 5; ++c) acc[q][c] = 0.0;
                }
                // fp32 x fp32 products are exact in fp64 and < 3000 fp64 additions lose ~1e-13 relative: the quotient is the
                // exact weighted mean to one fp32 rounding.  Membership does not depend on the order, so the lanes walk
                // cand[] as it lies (row order) rather than through the sorted keys.
                for (int j = lane; j < n; j += 64) {
                    const Cand c = cand[j];
                    const float o = c.cls * off_mul;
                    const float x1 = c.x1 + o, y1 = c.y1 + o, x2 = c.x2 + o, y2 = c.y2 + o;
                    const float area = (x2 - x1) * (y2 - y1);
                    const double w = (double)c.conf;                                                // :453
                    const double w0 = w * (double)c.x1, w1 = w * (double)c.y1;                      // :454, un-offset corners
                    const double w2 = w * (double)c.x2, w3 = w * (double)c.y2;
#pragma unroll
                    for (int q = 0; q < MB; ++q)
                        if (iou_tv(bx1[q], by1[q], bx2[q], by2[q], bar[q], x1, y1, x2, y2, area) > d.iou_thres) {   // :452
                            acc[q][0] += w; acc[q][1] += w0; acc[q][2] += w1; acc[q][3] += w2; acc[q][4] += w3;
                        }
                }
#pragma unroll
                for (int q = 0; q < MB; ++q) {
#pragma unroll
                    for (int c = 0; c < 5; ++c)
                        for (int m = 32; m > 0; m >>= 1) acc[q][c] += __shfl_xor(acc[q][c], m, 64);  // fixed order: run-to-run identical
                    if (lane == 0 && base + q < nkept) {
                        float* o = d.out + ((long)b * d.max_num + base + q) * 6;
                        o[0] = (float)(acc[q][1] / acc[q][0]); o[1] = (float)(acc[q][2] / acc[q][0]);
                        o[2] = (float)(acc[q][3] / acc[q][0]); o[3] = (float)(acc[q][4] / acc[q][0]);
                    }
                }
            }
        }
    }
}

}  // namespace nmsp
