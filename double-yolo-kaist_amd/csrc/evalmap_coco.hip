// Per-batch half of the COCO-protocol evaluation on the device: every detection of an evaluation batch is matched to the
// ground truth of its image and class at up to 16 IoU thresholds in up to 4 area ranges, one launch per batch, one
// workgroup of one wavefront per image.  The protocol is stated once, in include/dyk_hip.h (dyk_eval_match_coco); the
// accumulation stays on the host (other_utils.metrics.coco_accumulate).
//
// Replaces (reference): the per-image loop of train_utils/kaist_train_eval_utils.py:122-190 (scale_coords + round, three
// device-to-host copies, a dict per detection) and the per-image matching pycocotools runs on those dicts.
//
// dyk_eval_match's first pass (IoU and arg-max per detection, independent of the claims) is what this rule forbids: here a
// detection takes the best box that is still free at its (area, threshold), so the choice depends on every earlier
// detection of the class.  The decomposition:
//   1. the image's ground truth (fp32 x, y, w, h -- converted to fp64 exactly where it is used -- class, and one
//      ignore bit per area range) and its detections (corners as used, score, class) are staged in LDS;
//   2. ranks by counting, a lane per detection: `rank` among the detections of the class, `pos` among all of them; walking
//      by `pos` walks every class in rank order, and classes do not interact;
//   3. per detection in that order: all lanes compute its IoU with the boxes of its class, a lane per box in strides of 64,
//      and keep, in row order (ballot + popcount), the few that reach the smallest threshold; then lane a*T + t makes the
//      sequential decision for its own (a, t) over that short list against its own column of the claimed bits -- two
//      passes, non-ignored boxes first, ignored ones only while nothing is found;
//   4. two ballots carry the A x T decisions of the detection into dtm / dtig; lane a*T + t stores match[r][a][t].
// One wavefront, so there is no cross-wave step anywhere; the barriers below only order LDS writes before reads.
#pragma clang fp contract(off)
#include "dyk_common.h"
#include "box_scale.h"

namespace {

constexpr int MAX_GT = DYK_EVAL_MAX_GT, MAX_DET = DYK_EVAL_COCO_MAX_NUM;
constexpr uint16_t NONE16 = 0xffffu;

__global__ __launch_bounds__(DYK_WAVE) void eval_match_coco_kernel(DykEvalCocoDesc e) {
    __shared__ float s_g[MAX_GT][4];                             // gx, gy, gw, gh: fp32 values, exact in fp64
    __shared__ int s_gcls[MAX_GT];
    __shared__ uint8_t s_gig[MAX_GT];                            // bit a: ignored in area range a
    __shared__ uint32_t s_claim[MAX_GT / 32][DYK_WAVE];          // [word][lane a*T+t]: a lane's column, one bank each
    __shared__ double s_ciou[MAX_GT];                            // the candidates of one detection, in row order
    __shared__ uint16_t s_ck[MAX_GT];
    __shared__ float s_det[MAX_DET][4];
    __shared__ float s_score[MAX_DET];
    __shared__ int s_dcls[MAX_DET];
    __shared__ uint16_t s_rank[MAX_DET];
    __shared__ uint16_t s_order[MAX_DET];                        // pos -> detection
    __shared__ uint8_t s_done[MAX_DET];

    const int b = blockIdx.x, lane = threadIdx.x;
    int n = e.counts[b];
    if (n <= 0) return;                                          // (-1: an overflowed dyk_nms_rows image)
    if (n > e.max_num) n = e.max_num;                            // <= MAX_DET: checked before the launch
    const int r0 = e.rec_off[b], g0 = e.gt_off[b], g1 = e.gt_off[b + 1];
    const int ng = g1 - g0;
    if (r0 < 0 || (long)r0 + n > e.rec_cap || g0 < 0 || ng < 0 || g1 > e.nt || ng > MAX_GT) {
        if (lane == 0) e.err[1] = 1;                             // only ever set: every writer stores the same word
        return;
    }
    const int A = e.A, T = e.T;
    const float w0 = (float)e.shape0[2 * b], h0 = (float)e.shape0[2 * b + 1];

    // 1. ground truth (fp32, the converter's expressions), its ignore bits, the claimed bits
    for (int k = lane; k < ng; k += DYK_WAVE) {
        const float* t = e.targets + (long)(g0 + k) * 6;
        const float gx = (t[2] - 0.5f * t[4]) * w0, gy = (t[3] - 0.5f * t[5]) * h0, gw = t[4] * w0, gh = t[5] * h0;
        s_g[k][0] = gx; s_g[k][1] = gy; s_g[k][2] = gw; s_g[k][3] = gh;
        s_gcls[k] = (int)t[1];
        const double garea = (double)gw * (double)gh;
        uint32_t ig = 0;
        for (int a = 0; a < A; ++a) ig |= (garea < e.area[a][0] || garea > e.area[a][1]) ? 1u << a : 0u;
        s_gig[k] = (uint8_t)ig;
    }
    for (int i = lane; i < ((ng + 31) >> 5) * DYK_WAVE; i += DYK_WAVE) (&s_claim[0][0])[i] = 0u;

    float pad_x = 0.f, pad_y = 0.f, gain = 1.f;
    bool do_scale = false;
    if (e.unpad) {
        pad_x = e.unpad[4 * b]; pad_y = e.unpad[4 * b + 1]; gain = e.unpad[4 * b + 2];
        do_scale = e.unpad[4 * b + 3] != 0.f;
    }
    for (int i = lane; i < n; i += DYK_WAVE) {
        const float* d = e.out + ((long)b * e.max_num + i) * 6;
        float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3];
        if (do_scale) {
            unletterbox(x1, y1, x2, y2, pad_x, pad_y, gain);
            clip_box(x1, y1, x2, y2, w0, h0);
        }
        if (e.round_boxes) { x1 = rintf(x1); y1 = rintf(y1); x2 = rintf(x2); y2 = rintf(y2); }
        const int c = (int)d[5];
        s_det[i][0] = x1; s_det[i][1] = y1; s_det[i][2] = x2; s_det[i][3] = y2;
        s_score[i] = d[4];
        s_dcls[i] = c;
        s_order[i] = NONE16;
        s_done[i] = 0;
        const long r = (long)r0 + i;
        e.conf[r] = d[4];
        e.cls[r] = c;
        e.img[r] = e.img_base + b;
        float* rb = e.box + r * 4;
        rb[0] = x1; rb[1] = y1; rb[2] = x2; rb[3] = y2;
        e.darea[r] = (double)(x2 - x1) * (double)(y2 - y1);
        if (c < 0 || c >= e.nc) e.err[0] = 1;
    }
    __syncthreads();

    // 2. ranks by counting.  Scores that do not order (NaN) can give two detections one `pos`; the slot keeps one of them and
    // the other is finished in step 5, so every record is written exactly once whatever the scores are.
    for (int i = lane; i < n; i += DYK_WAVE) {
        const float s = s_score[i];
        const int c = s_dcls[i];
        int rank = 0, pos = 0;
        for (int j = 0; j < n; ++j) {
            const float sj = s_score[j];
            const int before = (sj > s || (sj == s && j < i)) ? 1 : 0;
            pos += before;
            rank += s_dcls[j] == c ? before : 0;
        }
        s_rank[i] = (uint16_t)rank;
        s_order[pos] = (uint16_t)i;                              // pos < n
        e.rank[(long)r0 + i] = rank;
    }
    __syncthreads();

    // lane a*T + t decides (a, t)
    const int AT = A * T;
    const bool decides = lane < AT;
    const int my_a = decides ? lane / T : 0, my_t = decides ? lane % T : 0;
    const double cap = 1.0 - 1e-10;
    const double my_thr = e.thr[my_t] < cap ? e.thr[my_t] : cap;
    const double my_lo = e.area[my_a][0], my_hi = e.area[my_a][1];
    double thr_min = cap;
    for (int t = 0; t < T; ++t) thr_min = e.thr[t] < thr_min ? e.thr[t] : thr_min;
    const uint64_t below = (1ull << lane) - 1ull;

    // 3. / 4. the detections in rank order
    for (int q = 0; q < n; ++q) {
        const int i = s_order[q];
        if (i >= n) continue;                                    // NONE16: an unordered score took this slot's owner elsewhere
        const int c = s_dcls[i];
        if (s_done[i] || s_rank[i] >= e.max_det || c < 0 || c >= e.nc) continue;   // uniform: step 5 writes these
        __syncthreads();                                         // the previous candidate list is consumed
        if (lane == 0) s_done[i] = 1;
        const float x1 = s_det[i][0], y1 = s_det[i][1], x2 = s_det[i][2], y2 = s_det[i][3];
        const double dx = x1, dy = y1, dw = (double)(x2 - x1), dh = (double)(y2 - y1);
        const double darea = dw * dh, dxe = dx + dw, dye = dy + dh;
        int ncand = 0;
        for (int k0 = 0; k0 < ng; k0 += DYK_WAVE) {
            const int k = k0 + lane;
            bool keep = false;
            double v = 0.0;
            if (k < ng && s_gcls[k] == c) {
                const double gx = s_g[k][0], gy = s_g[k][1], gw = s_g[k][2], gh = s_g[k][3];
                const double gxe = gx + gw, gye = gy + gh;
                const double w = (dxe < gxe ? dxe : gxe) - (dx > gx ? dx : gx);
                const double h = (dye < gye ? dye : gye) - (dy > gy ? dy : gy);
                if (!(w <= 0.0) && !(h <= 0.0)) {
                    const double inter = w * h;
                    v = inter / (darea + gw * gh - inter);
                }
                keep = !(v < thr_min);                           // below every threshold: no (a, t) can take it
            }
            const uint64_t m = __ballot(keep);
            if (keep) {
                const int p = ncand + __popcll(m & below);
                s_ck[p] = (uint16_t)k;
                s_ciou[p] = v;
            }
            ncand += __popcll(m);
        }
        __syncthreads();
        int m = -1;
        bool ig = false;
        if (decides) {
            double best = my_thr;
            for (int pass = 0; pass < 2 && m < 0; ++pass) {      // non-ignored boxes first; ignored ones only while m is none
                for (int p = 0; p < ncand; ++p) {
                    const int k = s_ck[p];
                    if (((s_gig[k] >> my_a) & 1) != pass) continue;
                    if ((s_claim[k >> 5][lane] >> (k & 31)) & 1u) continue;
                    const double v = s_ciou[p];
                    if (v < best) continue;
                    best = v;
                    m = k;
                }
                if (m >= 0) ig = pass != 0;
            }
            if (m >= 0) s_claim[m >> 5][lane] |= 1u << (m & 31);
            else ig = darea < my_lo || darea > my_hi;
        }
        const uint64_t bm = __ballot(m >= 0), bi = __ballot(ig);
        const long r = (long)r0 + i;
        if (lane < A) {
            const uint32_t field = (1u << T) - 1u;               // T <= 16, lane * T <= 48
            e.dtm[r * A + lane] = (uint32_t)(bm >> (lane * T)) & field;
            e.dtig[r * A + lane] = (uint32_t)(bi >> (lane * T)) & field;
        }
        if (decides) e.match[r * AT + lane] = (int16_t)m;
    }
    __syncthreads();

    // 5. what took no part: a rank >= max_det, a class outside [0, nc), a detection whose score did not order
    for (int i = lane; i < n; i += DYK_WAVE) {
        if (s_done[i]) continue;
        const long r = (long)r0 + i;
        for (int a = 0; a < A; ++a) { e.dtm[r * A + a] = 0u; e.dtig[r * A + a] = 0u; }
        for (int p = 0; p < AT; ++p) e.match[r * AT + p] = (int16_t)-1;
    }
}

}  // namespace

extern "C" int dyk_eval_match_coco(const DykEvalCocoDesc* e, void* stream) {
    if (!e || !e->out || !e->counts || !e->rec_off || !e->gt_off || !e->shape0 || !e->conf || !e->cls || !e->img ||
        !e->rank || !e->box || !e->darea || !e->dtm || !e->dtig || !e->match || !e->err)
        return DYK_ERR_ARG;
    if (e->B < 1 || e->max_num < 1 || e->max_num > DYK_EVAL_COCO_MAX_NUM || e->nc < 1 || e->T < 1 ||
        e->T > DYK_EVAL_MAX_THR || e->nt < 0 || e->rec_cap < 0 || (e->nt > 0 && !e->targets))
        return DYK_ERR_ARG;
    if (e->A < 1 || e->A > DYK_EVAL_MAX_AREA || e->A * e->T > DYK_WAVE || e->max_det < 1) return DYK_ERR_ARG;
    hipLaunchKernelGGL(eval_match_coco_kernel, dim3(e->B), dim3(DYK_WAVE), 0, (hipStream_t)stream, *e);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
