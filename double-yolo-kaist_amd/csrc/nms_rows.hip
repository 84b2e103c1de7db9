// Multi-label non-maximum suppression with a bounded workspace (dyk_nms_rows; the `multi_label` branch of reference
// build_utils/utils.py:422-424 in front of the same :430-431, :446-454 that nms.hip restates).  One 1024-thread workgroup per
// image, like nms_kernel, and the same phases 2 to 4 (nms_phases.h).  The candidate pass differs: nms_kernel gives a thread
// to every (row, class) pair -- N * nc / 1024 turns of three block barriers, every pair re-reading its row's header, a
// workspace for N * nc candidates.  Here:
//   1a. row survey   a thread per row reads w, h, obj; the alive rows (obj > conf_thres, 2 < w,h < 4096) are compacted in
//                    order into rowlist[] (wave ballot + per-wave counts in LDS);  ceil(N / 1024) turns, one barrier each
//                    (the per-wave counts are double-buffered and every thread keeps the running base in a register);
//   1b. count        a wavefront per alive row, the wavefronts taking rows round-robin, RB rows in flight each: the lanes read
//                    64 consecutive class scores per load, ballot conf = cls * obj > conf_thres (and the class filter), and
//                    the row's first lane stores the count;  no block barrier in the loop.  With nc <= 32 a row takes only
//                    W = pow2 >= nc lanes and a wavefront holds 64 / W rows side by side (a row per wavefront at nc = 2
//                    left 62 lanes idle: measured 917 us against the per-pair kernel's 686 us on 16 x 6100 alive rows);
//   1c. offsets      block-wide exclusive scan of the counts in place -> rowoff[], the image's n -> n_cand[b];
//                    n == 0: counts[b] = 0;  n > cand_cap: counts[b] = -1;  both return here, workgroup-uniform;
//   1d. write        the same walk again (the rows now come from L2): every passing lane stores its candidate and sort key
//                    at rowoff + earlier chunks of the row + popcount(ballot of the row's lanes below this one).
// The candidates are those of nms_kernel with multi_label = 1 in the same (row, class) order with the same bits: conf is
// one fp32 multiply, the corners are x - w / 2 etc. with FMA contraction off, every comparison is strict.
#include "nms_phases.h"

#pragma clang fp contract(off)

namespace {

using namespace nmsp;

constexpr int NW = NT / 64;    // wavefronts of the workgroup
constexpr int RB = 4;          // row groups one wavefront has in flight (the passes are bound by the latency of the row loads)

__device__ inline bool class_selected(const DykNmsRowsDesc& d, int cls) {         // :430-431
    if (d.n_classes <= 0) return true;
    bool in = false;
    for (int k = 0; k < d.n_classes; ++k) in |= (d.classes[k] == cls);
    return in;
}

// base + (counts of the wavefronts below wv) and the total of all wavefronts; every thread computes both
__device__ inline int wave_offset(const int* cnt, int wv, int& total) {
    int off = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
        const int c = cnt[q];
        off += q < wv ? c : 0;
        total += c;
    }
    return off;
}

template <bool MERGE>
__global__ __launch_bounds__(NT) void nms_rows_kernel(DykNmsRowsDesc d) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nc = d.no - 5;
    const unsigned long long below = (1ull << lane) - 1ull;
    long P = 1;
    while (P < d.cand_cap) P <<= 1;
    char* wsb = (char*)d.ws + (size_t)b * d.ws_per_image;
    unsigned long long* keys = (unsigned long long*)wsb;               // [P]
    Cand* cand = (Cand*)(wsb + P * sizeof(unsigned long long));        // [cand_cap]
    int* rowlist = (int*)(wsb + ws_bytes(d.cand_cap));                 // [N] alive rows, ascending
    int* rowoff = rowlist + d.N;                                       // [N] candidates per alive row, then their prefix sum
    const float* pred = d.pred + (long)b * d.N * d.no;

    __shared__ int wave_cnt[2][NW];
    __shared__ Kept kept;

    // ---------------------------------------------------------------- 1a. row survey
    int nalive = 0, turn = 0;
    for (long start = 0; start < d.N; start += NT, turn ^= 1) {
        const long row = start + tid;
        bool alive = false;
        if (row < d.N) {
            const float* x = pred + row * d.no;
            alive = x[4] > d.conf_thres && x[2] > 2.f && x[2] < 4096.f && x[3] > 2.f && x[3] < 4096.f;   // :408-409
        }
        const unsigned long long m = __ballot(alive);
        if (lane == 0) wave_cnt[turn][wv] = __popcll(m);
        __syncthreads();       // (turn t + 2 rewrites this buffer only behind the barrier of turn t + 1: every read is done)
        int total;
        const int off = nalive + wave_offset(wave_cnt[turn], wv, total);
        if (alive) rowlist[off + __popcll(m & below)] = (int)row;
        nalive += total;
    }
    __syncthreads();           // rowlist[] is complete; wave_cnt is free again
    // ---------------------------------------------------------------- 1b. count
    // W lanes per row: the power of two >= nc, 64 at the most (then the row's classes go by in chunks of 64); a wavefront
    // holds G = 64 / W rows side by side, RB times.  gmask = the lanes of this lane's row.
    int sh = 1;
    while ((1 << sh) < nc && sh < 6) ++sh;
    const int W = 1 << sh, G = 64 >> sh;
    const int sub = lane >> sh, cl = lane & (W - 1);
    const unsigned long long gmask = sh == 6 ? ~0ull : ((1ull << W) - 1ull) << (sub * W);
    const unsigned long long gbelow = gmask & below;
    for (int i0 = wv * RB * G; i0 < nalive; i0 += NW * RB * G) {
        const float* x[RB];
        float obj[RB];
        int cnt[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            x[r] = pred + (long)rowlist[min(i0 + r * G + sub, nalive - 1)] * d.no;   // (past the end: recomputed, not stored)
            cnt[r] = 0;
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) obj[r] = x[r][4];
        for (int c0 = 0; c0 < nc; c0 += W) {
            const int cls = c0 + cl;
            const bool in = cls < nc && class_selected(d, cls);
            float v[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) v[r] = cls < nc ? x[r][5 + cls] : 0.f;
#pragma unroll
            for (int r = 0; r < RB; ++r) cnt[r] += __popcll(__ballot(in && v[r] * obj[r] > d.conf_thres) & gmask);   // :416, :423
        }
#pragma unroll
        for (int r = 0; r < RB; ++r)
            if (cl == 0 && i0 + r * G + sub < nalive) rowoff[i0 + r * G + sub] = cnt[r];
    }
    __syncthreads();
    // ---------------------------------------------------------------- 1c. offsets
    int n = 0;
    turn = 0;
    for (int start = 0; start < nalive; start += NT, turn ^= 1) {
        const int i = start + tid;
        const int v = i < nalive ? rowoff[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wave_cnt[turn][wv] = inc;
        __syncthreads();
        int total;
        const int off = n + wave_offset(wave_cnt[turn], wv, total);
        if (i < nalive) rowoff[i] = off + inc - v;
        n += total;
    }
    if (tid == 0) d.n_cand[b] = n;
    if (n == 0 || n > d.cand_cap) {                // workgroup-uniform: every thread summed the same LDS words
        if (tid == 0) d.counts[b] = n == 0 ? 0 : -1;
        return;
    }
    __syncthreads();           // rowoff[] is complete
    // ---------------------------------------------------------------- 1d. write
    for (int i0 = wv * RB * G; i0 < nalive; i0 += NW * RB * G) {
        const float* x[RB];
        int row[RB], off[RB];
        float obj[RB], x1[RB], y1[RB], x2[RB], y2[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = min(i0 + r * G + sub, nalive - 1);
            row[r] = rowlist[i];
            off[r] = rowoff[i];
            x[r] = pred + (long)row[r] * d.no;
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float cx = x[r][0], cy = x[r][1], w = x[r][2], h = x[r][3];
            obj[r] = x[r][4];
            x1[r] = cx - w / 2; y1[r] = cy - h / 2;                           // xywh2xyxy :50-57
            x2[r] = cx + w / 2; y2[r] = cy + h / 2;
        }
        for (int c0 = 0; c0 < nc; c0 += W) {
            const int cls = c0 + cl;
            const bool in = cls < nc && class_selected(d, cls);
            float v[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) v[r] = cls < nc ? x[r][5 + cls] : 0.f;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const float conf = v[r] * obj[r];                             // :416
                const bool ok = in && conf > d.conf_thres;                    // :423
                const unsigned long long m = __ballot(ok);
                const int o = off[r] + __popcll(m & gbelow);
                if (ok && i0 + r * G + sub < nalive && o < d.cand_cap) {      // (o < n <= cand_cap by the count; never past the room)
                    Cand c;
                    c.x1 = x1[r]; c.y1 = y1[r]; c.x2 = x2[r]; c.y2 = y2[r];
                    c.conf = conf; c.cls = (float)cls; c.row = row[r];
                    cand[o] = c;
                    keys[o] = sort_key(conf, o);
                }
                off[r] += __popcll(m & gmask);
            }
        }
    }
    sort_suppress_merge<MERGE>(d, keys, cand, n, kept);                 // 2. sort, 3. suppression, 4. merge
}

}  // namespace

extern "C" int64_t dyk_nms_rows_workspace_bytes(int32_t N, int32_t cand_cap) {
    return ws_bytes(cand_cap) + (8L * N + 255) / 256 * 256;
}

extern "C" int dyk_nms_rows(const DykNmsRowsDesc* d, int32_t flags, void* stream) {
    if (flags & ~DYK_NMS_MERGE) return DYK_ERR_ARG;
    if (!d || !d->pred || !d->out || !d->out_rows || !d->counts || !d->ws || !d->n_cand) return DYK_ERR_ARG;
    if (d->B <= 0 || d->N <= 0 || d->no < 6 || d->max_num <= 0 || d->max_num > MAX_KEEP) return DYK_ERR_ARG;
    if (d->n_classes < 0 || d->n_classes > 16) return DYK_ERR_ARG;
    if (!d->multi_label || d->no < 7) return DYK_ERR_ARG;                // best-class calls stay with dyk_nms_ex
    if ((int64_t)d->N * (d->no - 5) > 0x7fffffffLL) return DYK_ERR_ARG;  // the candidate count is an int32
    if (d->cand_cap < 1) return DYK_ERR_ARG;
    if (d->ws_per_image < dyk_nms_rows_workspace_bytes(d->N, d->cand_cap)) return DYK_ERR_ARG;
    if (!(d->conf_thres >= 0.f)) return DYK_ERR_ARG;     // score bits must be monotonic (positive floats)
    if (flags & DYK_NMS_MERGE)
        hipLaunchKernelGGL(nms_rows_kernel<true>, dim3(d->B), dim3(NT), 0, (hipStream_t)stream, *d);
    else
        hipLaunchKernelGGL(nms_rows_kernel<false>, dim3(d->B), dim3(NT), 0, (hipStream_t)stream, *d);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
