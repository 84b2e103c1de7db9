// Per-image detection filtering + greedy non-maximum suppression on the device.
// Replaces non_max_suppression (reference build_utils/utils.py:387-464) together with the
// torchvision.ops.nms call inside it (:448).  One 1024-thread workgroup per image:
//   1. candidate generation in row order (ordered compaction by wave ballot + prefix):
//      obj > conf_thres, 2 < w,h < 4096, conf = obj*cls, best class (or every class when
//      multi_label), conf > conf_thres, optional class filter; boxes converted centre->corner;
//   2. stable descending sort by score: bitonic sort of 64-bit keys (inverted score bits | index);
//   3. greedy suppression in score order, 64 candidates per step on one wavefront: each lane tests
//      its candidate against the kept list (LDS), then the wave resolves the chunk internally with
//      cross-lane broadcasts; stops at max_num kept boxes (the reference truncates [:max_num]);
//   4. (DYK_NMS_MERGE only, 1 < n < 3000) merge-NMS (:450-454): every kept box becomes the score-weighted mean of all
//      candidates whose IoU with it exceeds iou_thres.  Kept boxes are dealt round-robin, four at a time, to the 16 wavefronts; lanes
//      stride over the candidates with fp64 accumulators and a fixed-order butterfly finishes each box.
// IoU arithmetic follows torchvision's CPU kernel operation for operation in fp32 (no FMA
// contraction) so that the keep-set is bit-identical for identical inputs.
#include "dyk_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 1024;
constexpr int MAX_KEEP = 512;
constexpr int MB = 4;          // kept boxes one wavefront merges per pass over the candidates

struct Cand {
    float x1, y1, x2, y2, conf, cls;
    int row;
};

__device__ inline float iou_tv(float ax1, float ay1, float ax2, float ay2, float aarea, float bx1, float by1, float bx2,
                               float by2, float barea) {
    const float xx1 = fmaxf(ax1, bx1), yy1 = fmaxf(ay1, by1);
    const float xx2 = fminf(ax2, bx2), yy2 = fminf(ay2, by2);
    const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
    const float inter = w * h;
    return inter / ((aarea + barea) - inter);
}

// MERGE = false is the plain kernel: every merge statement sits under `if constexpr (MERGE)`.
template <bool MERGE>
__global__ __launch_bounds__(NT) void nms_kernel(DykNmsDesc d) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nc = d.no - 5;
    const bool multi = d.multi_label && nc > 1;
    const long cap = (long)d.N * (multi ? nc : 1);
    long P = 1;
    while (P < cap) P <<= 1;
    char* wsb = (char*)d.ws + (size_t)b * d.ws_per_image;
    unsigned long long* keys = (unsigned long long*)wsb;               // [P]
    Cand* cand = (Cand*)(wsb + P * sizeof(unsigned long long));        // [cap]
    const float* pred = d.pred + (long)b * d.N * d.no;

    __shared__ int wave_cnt[NT / 64];
    __shared__ int base_s;
    __shared__ float kx1[MAX_KEEP], ky1[MAX_KEEP], kx2[MAX_KEEP], ky2[MAX_KEEP], kar[MAX_KEEP];
    __shared__ int nkept_s;
    if (tid == 0) { base_s = 0; nkept_s = 0; }
    __syncthreads();

    // ---------------------------------------------------------------- 1. candidates
    for (long start = 0; start < cap; start += NT) {
        const long idx = start + tid;
        bool ok = false;
        Cand c;
        if (idx < cap) {
            const int row = (int)(multi ? idx / nc : idx);
            const float* x = pred + (long)row * d.no;
            const float obj = x[4];
            if (obj > d.conf_thres && x[2] > 2.f && x[2] < 4096.f && x[3] > 2.f && x[3] < 4096.f) {   // :408-409
                float conf;
                int cls;
                if (multi) {
                    cls = (int)(idx - (long)row * nc);
                    conf = x[5 + cls] * obj;                                  // :416
                } else {
                    conf = x[5] * obj;
                    cls = 0;
                    for (int k = 1; k < nc; ++k) {                            // first maximum wins
                        const float v = x[5 + k] * obj;
                        if (v > conf) { conf = v; cls = k; }
                    }
                }
                ok = conf > d.conf_thres;                                     // :423 / :427
                if (ok && d.n_classes > 0) {                                  // :430-431
                    bool in = false;
                    for (int k = 0; k < d.n_classes; ++k) in |= (d.classes[k] == cls);
                    ok = in;
                }
                if (ok) {
                    c.x1 = x[0] - x[2] / 2; c.y1 = x[1] - x[3] / 2;           // xywh2xyxy :50-57
                    c.x2 = x[0] + x[2] / 2; c.y2 = x[1] + x[3] / 2;
                    c.conf = conf; c.cls = (float)cls; c.row = row;
                }
            }
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int off = base_s;
        for (int q = 0; q < wv; ++q) off += wave_cnt[q];
        if (ok) {
            const int o = off + __popcll(m & ((1ull << lane) - 1ull));
            cand[o] = c;
            const unsigned int sb = __float_as_uint(c.conf);                  // conf > 0: bits are monotonic
            keys[o] = ((unsigned long long)(0xFFFFFFFFu - sb) << 32) | (unsigned int)o;
        }
        __syncthreads();
        if (tid == 0) { int s = 0; for (int q = 0; q < NT / 64; ++q) s += wave_cnt[q]; base_s += s; }
        __syncthreads();
    }
    const int n = base_s;
    if (n == 0) {
        if (tid == 0) d.counts[b] = 0;
        return;
    }
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
                    if (iou_tv(kx1[k], ky1[k], kx2[k], ky2[k], kar[k], x1, y1, x2, y2, area) > d.iou_thres) alive = false;
            }
            for (int s = 0; s < 64 && nkept < max_keep; ++s) {
                const bool sa = __shfl((int)alive, s, 64) != 0;
                if (!sa) continue;
                const float sx1 = __shfl(x1, s, 64), sy1 = __shfl(y1, s, 64), sx2 = __shfl(x2, s, 64), sy2 = __shfl(y2, s, 64);
                const float sar = __shfl(area, s, 64);
                if (lane == s) {
                    kx1[nkept] = x1; ky1[nkept] = y1; kx2[nkept] = x2; ky2[nkept] = y2; kar[nkept] = area;
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
            if constexpr (MERGE) nkept_s = nkept;
        }
    }
    // ---------------------------------------------------------------- 4. merge (all 16 wavefronts)
    if constexpr (MERGE) {
        __syncthreads();                           // kept list, nkept_s and wave 0's out[] rows are complete (n is uniform)
        if (n > 1 && n < 3000) {                   // :450, both strict; n counts candidates, not rows
            const int nkept = nkept_s;
            const float off_mul = d.agnostic ? 0.f : 4096.f;
            // MB kept boxes per pass over the candidates: the loop is bound by the latency of the cand[] load, which the
            // MB boxes share (measured, 16 x (n = 2999, 100 kept): 105 us with one box per pass, 76 us with four)
            for (int base = wv * MB; base < nkept; base += (NT / 64) * MB) {
                float bx1[MB], by1[MB], bx2[MB], by2[MB], bar[MB];                                  // boxes[i[k]], offset
                double acc[MB][5];
#pragma unroll
                for (int q = 0; q < MB; ++q) {
                    const int k = min(base + q, nkept - 1);                                         // (past the end: recomputed, not written)
                    bx1[q] = kx1[k]; by1[q] = ky1[k]; bx2[q] = kx2[k]; by2[q] = ky2[k]; bar[q] = kar[k];
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

}  // namespace

extern "C" int64_t dyk_nms_workspace_bytes(int32_t N, int32_t no, int32_t multi_label) {
    const int nc = no - 5;
    const long cap = (long)N * ((multi_label && nc > 1) ? nc : 1);
    long P = 1;
    while (P < cap) P <<= 1;
    const long bytes = P * 8 + cap * (long)sizeof(Cand);
    return (bytes + 255) / 256 * 256;
}

extern "C" int dyk_nms_ex(const DykNmsDesc* d, int32_t flags, void* stream) {
    if (flags & ~DYK_NMS_MERGE) return DYK_ERR_ARG;
    if (!d || !d->pred || !d->out || !d->out_rows || !d->counts || !d->ws) return DYK_ERR_ARG;
    if (d->B <= 0 || d->N <= 0 || d->no < 6 || d->max_num <= 0 || d->max_num > MAX_KEEP) return DYK_ERR_ARG;
    if (d->n_classes < 0 || d->n_classes > 16) return DYK_ERR_ARG;
    if (d->ws_per_image < dyk_nms_workspace_bytes(d->N, d->no, d->multi_label)) return DYK_ERR_ARG;
    if (!(d->conf_thres >= 0.f)) return DYK_ERR_ARG;     // score bits must be monotonic (positive floats)
    if (flags & DYK_NMS_MERGE)
        hipLaunchKernelGGL(nms_kernel<true>, dim3(d->B), dim3(NT), 0, (hipStream_t)stream, *d);
    else
        hipLaunchKernelGGL(nms_kernel<false>, dim3(d->B), dim3(NT), 0, (hipStream_t)stream, *d);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_nms(const DykNmsDesc* d, void* stream) { return dyk_nms_ex(d, 0, stream); }
