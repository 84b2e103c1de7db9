// Per-batch half of the multi-class AP / mAP evaluation on the device: every detection of an evaluation batch is matched
// to the ground truth of its image and class at up to 16 IoU thresholds, one launch per batch, one wavefront per image.
//
// Replaces (reference): other_utils/metrics.py box_iou :62-79 and the matching loop of compute_ap_lamr :81-130 (run per
// class), the caller's per-image loop evaluate.py:76-106 (scale_coords launch, three device-to-host copies, a dict per
// detection) and scale_coords / clip_coords build_utils/utils.py:60-92.  The curve arithmetic stays on the host
// (other_utils.metrics.compute_map): it runs once per epoch on three small arrays.
//
// Every decision is the host evaluator's decision because every type is its type: ground truth fp32 -> int32 by truncation,
// detection area fp32, ground-truth area int32, the rest fp64 after exact conversion (numpy's promotion of float32 with
// int32), separate IEEE operations in numpy's order -- no FMA anywhere in this file.
//
// Latency-bound and tiny.  The image's ground truth (<= 1024 boxes, 20 KB) and its detections (chunks of 128) are staged in
// LDS first, so nothing below waits for a global load.  Two passes per chunk: a lane per detection finds its best box
// (IoU and argmax do not depend on the claims), then lane t walks the detections in NMS order for threshold t against its
// own row of the claimed bits (T * 32 words of LDS) -- the only sequential part, without a cross-lane step but one ballot.
#pragma clang fp contract(off)
#include "dyk_common.h"
#include "box_scale.h"

namespace {

constexpr int DET_CHUNK = 128;

__global__ __launch_bounds__(DYK_WAVE) void eval_match_kernel(DykEvalMatchDesc e) {
    __shared__ int s_gt[DYK_EVAL_MAX_GT][4];                     // int32 corners, as `.astype(np.int32)` leaves them
    __shared__ int s_gcls[DYK_EVAL_MAX_GT];
    __shared__ uint32_t s_claimed[DYK_EVAL_MAX_THR][DYK_EVAL_MAX_GT / 32];
    __shared__ float s_det[DET_CHUNK][4];
    __shared__ int s_dcls[DET_CHUNK];
    __shared__ double s_best[DET_CHUNK];                         // per detection: the largest IoU, its box (or -1), the TP bits
    __shared__ int s_bk[DET_CHUNK];
    __shared__ uint32_t s_mask[DET_CHUNK];

    const int b = blockIdx.x, lane = threadIdx.x;
    int n = e.counts[b];
    if (n <= 0) return;                                          // (-1: an overflowed dyk_nms_rows image)
    if (n > e.max_num) n = e.max_num;
    const int r0 = e.rec_off[b], g0 = e.gt_off[b], g1 = e.gt_off[b + 1];
    const int ng = g1 - g0;
    if (r0 < 0 || (long)r0 + n > e.rec_cap || g0 < 0 || ng < 0 || g1 > e.nt || ng > DYK_EVAL_MAX_GT) {
        if (lane == 0) e.err[1] = 1;                             // only ever set: every writer stores the same word
        return;
    }
    const int w0i = e.shape0[2 * b], h0i = e.shape0[2 * b + 1];
    const float w0 = (float)w0i, h0 = (float)h0i;

    // ground truth -> absolute int32 corners (metrics._absolute_xyxy, then astype(int32))
    for (int k = lane; k < ng; k += DYK_WAVE) {
        const float* t = e.targets + (long)(g0 + k) * 6;
        const float xc = t[2] * w0, yc = t[3] * h0, bw = t[4] * w0, bh = t[5] * h0;
        const float x1 = xc - bw / 2.f, y1 = yc - bh / 2.f;
        const float x2 = bw + x1, y2 = bh + y1;
        s_gt[k][0] = (int)x1; s_gt[k][1] = (int)y1; s_gt[k][2] = (int)x2; s_gt[k][3] = (int)y2;
        s_gcls[k] = (int)t[1];
    }
    for (int i = lane; i < e.T * (DYK_EVAL_MAX_GT / 32); i += DYK_WAVE) (&s_claimed[0][0])[i] = 0u;

    const double my_thr = e.thr[lane < e.T ? lane : 0];          // lane t decides threshold t
    float pad_x = 0.f, pad_y = 0.f, gain = 1.f;
    bool do_scale = false;
    if (e.unpad) {
        pad_x = e.unpad[4 * b]; pad_y = e.unpad[4 * b + 1]; gain = e.unpad[4 * b + 2];
        do_scale = e.unpad[4 * b + 3] != 0.f;
    }

    for (int c0 = 0; c0 < n; c0 += DET_CHUNK) {
        const int nchunk = n - c0 < DET_CHUNK ? n - c0 : DET_CHUNK;
        __syncthreads();                                         // the previous chunk is consumed; the first: s_gt is written
        for (int i = lane; i < nchunk; i += DYK_WAVE) {
            const float* d = e.out + ((long)b * e.max_num + c0 + i) * 6;
            float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3];
            if (do_scale) {
                unletterbox(x1, y1, x2, y2, pad_x, pad_y, gain);
                clip_box(x1, y1, x2, y2, w0, h0);
            }
            const int c = (int)d[5];
            s_det[i][0] = x1; s_det[i][1] = y1; s_det[i][2] = x2; s_det[i][3] = y2;
            s_dcls[i] = c;
            const long r = (long)r0 + c0 + i;
            e.conf[r] = d[4];
            e.cls[r] = c;
            float* rb = e.box + r * 4;
            rb[0] = x1; rb[1] = y1; rb[2] = x2; rb[3] = y2;
        }
        __syncthreads();
        // IoU and argmax do not depend on what is claimed: a lane per detection, boxes in ascending order (a strict `>` keeps
        // the first maximum, np.argmax)
        for (int i = lane; i < nchunk; i += DYK_WAVE) {
            const float x1 = s_det[i][0], y1 = s_det[i][1], x2 = s_det[i][2], y2 = s_det[i][3];
            const int c = s_dcls[i];
            const bool bad = c < 0 || c >= e.nc;                                 // no match, and the launch's error flag
            const float a1f = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);                 // float32 area
            const double a1 = (double)a1f, dx1 = x1, dy1 = y1, dx2 = x2, dy2 = y2;
            double best = -__builtin_inf();
            int bk = -1;
            for (int k = 0; k < ng; ++k) {
                if (bad || s_gcls[k] != c) continue;
                const int gx1 = s_gt[k][0], gy1 = s_gt[k][1], gx2 = s_gt[k][2], gy2 = s_gt[k][3];
                const int a2 = (gx2 - gx1 + 1) * (gy2 - gy1 + 1);                // int32 area (wraps like numpy's)
                const double fx1 = gx1, fy1 = gy1, fx2 = gx2, fy2 = gy2;
                double w = (dx2 < fx2 ? dx2 : fx2) - (dx1 > fx1 ? dx1 : fx1) + 1.0;
                double h = (dy2 < fy2 ? dy2 : fy2) - (dy1 > fy1 ? dy1 : fy1) + 1.0;
                w = w < 0.0 ? 0.0 : (w > 1e5 ? 1e5 : w);
                h = h < 0.0 ? 0.0 : (h > 1e5 ? 1e5 : h);
                const double inter = w * h;
                const double v = inter / (a1 + (double)a2 - inter);
                if (v > best) { best = v; bk = k; }
            }
            s_best[i] = bk >= 0 ? best : 0.0;
            s_bk[i] = bk;
            if (bad) e.err[0] = 1;
        }
        __syncthreads();
        // the claims are sequential in the detections and independent between thresholds: lane t owns row t of the claimed
        // bits and walks the chunk in NMS order; a ballot gathers the T decisions of one detection into its mask
        for (int i = 0; i < nchunk; ++i) {
            const int bk = s_bk[i];
            bool tp = false;
            if (lane < e.T && bk >= 0) {
                const uint32_t bit = 1u << (bk & 31), wd = s_claimed[lane][bk >> 5];
                if (s_best[i] >= my_thr && !(wd & bit)) {
                    s_claimed[lane][bk >> 5] = wd | bit;
                    tp = true;
                }
            }
            const uint32_t mask = (uint32_t)__ballot(tp);
            if (lane == 0) s_mask[i] = mask;
        }
        __syncthreads();
        for (int i = lane; i < nchunk; i += DYK_WAVE) {
            const long r = (long)r0 + c0 + i;
            e.tp_mask[r] = s_mask[i];
            e.match[r] = s_bk[i] >= 0 ? g0 + s_bk[i] : -1;
            e.iou[r] = s_best[i];
        }
    }
}

}  // namespace

extern "C" int dyk_eval_match(const DykEvalMatchDesc* e, void* stream) {
    if (!e || !e->out || !e->counts || !e->rec_off || !e->gt_off || !e->shape0 || !e->conf || !e->cls || !e->tp_mask ||
        !e->match || !e->iou || !e->box || !e->err)
        return DYK_ERR_ARG;
    if (e->B < 1 || e->max_num < 1 || e->nc < 1 || e->T < 1 || e->T > DYK_EVAL_MAX_THR || e->nt < 0 || e->rec_cap < 0 ||
        (e->nt > 0 && !e->targets))
        return DYK_ERR_ARG;
    hipLaunchKernelGGL(eval_match_kernel, dim3(e->B), dim3(DYK_WAVE), 0, (hipStream_t)stream, *e);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
