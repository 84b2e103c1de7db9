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
#include "nms_phases.h"

#pragma clang fp contract(off)

namespace {

using namespace nmsp;          // NT, MAX_KEEP, Cand, Kept, sort_key, sort_suppress_merge: phases 2 to 4 live in nms_phases.h

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
    __shared__ Kept kept;
    if (tid == 0) base_s = 0;
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
            keys[o] = sort_key(c.conf, o);
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
    sort_suppress_merge<MERGE>(d, keys, cand, n, kept);                 // 2. sort, 3. suppression, 4. merge
}

}  // namespace

extern "C" int64_t dyk_nms_workspace_bytes(int32_t N, int32_t no, int32_t multi_label) {
    const int nc = no - 5;
    return ws_bytes((long)N * ((multi_label && nc > 1) ? nc : 1));
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
