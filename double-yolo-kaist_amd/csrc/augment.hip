// dyk_augment_pairs: mosaic canvas, affine warp, HSV jitter and left-right flip of image pairs in one launch (reference
// build_utils/kaist_dataset.py: load_quadra_images, random_affine, augment_hsv, the flip of __getitem__).  The rule is stated
// once, in include/dyk_hip.h; tests/augment_ref.py restates it in plain numpy and the outputs are equal bit for bit.
//   grid   (strips of AUG_ROWS = 2 output rows, B images, 2 streams); one workgroup owns a strip of one output image of one stream
//   thread four consecutive output pixels of all three planes: the canvas look-up of a tap is shared by the planes, the HSV
//          stage needs the three together, and each plane gets one dword store (byte stores when Wo % 4 != 0 or dst is unaligned)
//   LDS    the image's 768-byte table and the two 256-entry division tables (2 816 bytes, static; filled only when there is a table)
//   taps   plain byte loads through the (at most four, wave-uniform) rectangles; no staging, no atomics, no scratch
// fp64 / fp32: every multiply and add of the rule is an operation of its own; the library is built with -ffp-contract=on, so
// contraction is switched off for this file by pragma (as in clahe.hip).
#include "dyk_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_THREADS = 256;
// output rows of one workgroup: chosen by measurement, DESIGN.md section 19 (dyk_augment_pairs_rows lets the probe sweep it)
constexpr int AUG_ROWS = 2;
constexpr int AUG_MAX_SIZE = 16384;          // every size of the descriptor
constexpr int AUG_RECTS = 4;

struct AugArgs {
    const uint8_t* src[2];
    uint8_t* dst[2];
    int N, B, H, W, Hc, Wc, Ho, Wo;
    const int32_t* rects;
    const double* minv;
    const uint8_t* luts;
    const uint8_t* flip;
    int vec4;                                // Wo % 4 == 0 and both dst bases 4-byte aligned: dword stores
    int rows;                                // output rows of one workgroup
};

// the rectangles of one image, checked: the kernel reads src only through these
struct AugCanvas {
    int x1[AUG_RECTS], y1[AUG_RECTS], x2[AUG_RECTS], y2[AUG_RECTS];
    long long off[AUG_RECTS];                // canvas (y, x) of rectangle k is src[off[k] + y*W + x], plane 0
    int n;
};

// round half to even of num / den for positive integers: the fp64 rn((255 << 12) / (1.0 * i)) of the rule without fp64 (the
// quotient of these tables is never within 1/512 of a tie unless it is one, so the double rounding of the fp64 form is none)
__device__ inline int div_rn(int num, int den) {
    const int q = num / den, r = num - q * den;
    return q + (int)(2 * r > den || (2 * r == den && (q & 1)));
}

// rn of the rule: round half to even to int32, saturating (NaN -> INT32_MIN; an admitted call never saturates)
__device__ inline int rn_i32(double v) {
    double r = rint(v);
    r = fmax(r, -2147483648.0);
    r = fmin(r, 2147483647.0);
    return (int)r;
}

__device__ inline uint32_t sat_rint_u8(float v) {
    const float r = rintf(v);                // half to even
    return (uint32_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

// one canvas tap of the three planes; 0 outside every rectangle
__device__ inline void canvas3(const AugCanvas& cv, const uint8_t* src, int W, size_t plane, int y, int x,
                               int& c0, int& c1, int& c2) {
    c0 = c1 = c2 = 0;
    bool hit = false;
    long long off = 0;
#pragma unroll
    for (int k = AUG_RECTS - 1; k >= 0; --k) {                   // downwards, so that the first rectangle that holds it wins
        const bool in = k < cv.n && x >= cv.x1[k] && x < cv.x2[k] && y >= cv.y1[k] && y < cv.y2[k];
        off = in ? cv.off[k] : off;                              // selects on constant indices: the records stay in registers
        hit = hit || in;
    }
    if (hit) {
        const uint8_t* p = src + (off + (long long)y * W + x);
        c0 = p[0];
        c1 = p[plane];
        c2 = p[2 * plane];
    }
}

// (c) of the rule on one pixel (planes R, G, B)
__device__ inline void hsv_jitter(const uint8_t* lut, const int* sdiv, const int* hdiv, int& r, int& g, int& b) {
    const int v = max(r, max(g, b)), vmin = min(r, min(g, b)), diff = v - vmin;
    const int s = (diff * sdiv[v] + 2048) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * hdiv[diff] + 2048) >> 12;       // arithmetic shift: h may be negative here
    if (h < 0) h += 180;
    const int h2 = lut[h], s2 = lut[256 + s], v2 = lut[512 + v];
    const float vf = (float)v2 * (1.f / 255.f);
    if (s2 == 0) {
        r = g = b = (int)sat_rint_u8(vf * 255.f);
        return;
    }
    const float hf = (float)h2 * (6.f / 180.f), sf = (float)s2 * (1.f / 255.f);
    int sector = (int)floorf(hf);
    const float f = hf - (float)sector;
    sector = min(sector, 5);                 // a table hue above 179: the rule takes sector 5
    const float t0 = vf, t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * f), t3 = vf * (1.f - sf * (1.f - f));
    float bf, gf, rf;
    switch (sector) {
    case 0: bf = t1; gf = t3; rf = t0; break;
    case 1: bf = t1; gf = t0; rf = t2; break;
    case 2: bf = t3; gf = t0; rf = t1; break;
    case 3: bf = t0; gf = t2; rf = t1; break;
    case 4: bf = t0; gf = t1; rf = t3; break;
    default: bf = t2; gf = t1; rf = t0; break;
    }
    r = (int)sat_rint_u8(rf * 255.f);
    g = (int)sat_rint_u8(gf * 255.f);
    b = (int)sat_rint_u8(bf * 255.f);
}

template <bool WARP>
__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(const AugArgs a) {
    __shared__ uint8_t lut[3 * 256];
    __shared__ int sdiv[256], hdiv[256];
    const int tid = threadIdx.x, b = blockIdx.y, stream = blockIdx.z;
    const bool jitter = a.luts != nullptr;   // uniform over the launch
    if (jitter) {
        const uint8_t* t = a.luts + (size_t)b * 768;
        for (int i = tid; i < 768; i += AUG_THREADS) lut[i] = t[i];
        sdiv[tid] = tid ? div_rn(255 << 12, tid) : 0;
        hdiv[tid] = tid ? div_rn(180 << 12, 6 * tid) : 0;
        __syncthreads();
    }
    const uint8_t* src = a.src[stream];                         // (no __restrict__: the jitter alone may run with dst == src)
    uint8_t* dst = a.dst[stream];
    const int W = a.W, H = a.H, Wo = a.Wo, Ho = a.Ho;
    const size_t plane = (size_t)H * W, oplane = (size_t)Ho * Wo;

    // the rectangles of image b: clipped to the canvas, and kept only when every pixel of them lies inside its source image
    AugCanvas cv;
    cv.n = 0;
#pragma unroll
    for (int k = 0; k < AUG_RECTS; ++k) { cv.x1[k] = cv.y1[k] = cv.x2[k] = cv.y2[k] = 0; cv.off[k] = 0; }
    if (a.rects) {
        const int32_t* q = a.rects + (size_t)b * AUG_RECTS * 8;
#pragma unroll
        for (int k = 0; k < AUG_RECTS; ++k) {
            const int x1 = max(q[8 * k], 0), y1 = max(q[8 * k + 1], 0), x2 = min(q[8 * k + 2], a.Wc), y2 = min(q[8 * k + 3], a.Hc);
            const int s = q[8 * k + 4];
            const long long dx = q[8 * k + 5], dy = q[8 * k + 6];
            const bool ok = x2 > x1 && y2 > y1 && s >= 0 && s < a.N && x1 - dx >= 0 && x2 - dx <= W && y1 - dy >= 0 && y2 - dy <= H;
            if (ok) {                                            // (slot k stays empty otherwise: constant indices, no scratch)
                cv.x1[k] = x1; cv.y1[k] = y1; cv.x2[k] = x2; cv.y2[k] = y2;
                cv.off[k] = ((long long)s * 3 * H - dy) * W - dx;
            }
        }
        cv.n = AUG_RECTS;
    } else {
        cv.n = 1;
        cv.x2[0] = W; cv.y2[0] = H;
        cv.off[0] = (long long)b * 3 * H * W;                    // b < N: the entry refuses B > N without rects
    }

    double m0 = 1.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 1.0, m5 = 0.0;
    if (WARP) {
        const double* m = a.minv + (size_t)b * 6;
        m0 = m[0]; m1 = m[1]; m2 = m[2]; m3 = m[3]; m4 = m[4]; m5 = m[5];
    }
    const bool flip = a.flip && a.flip[b];
    const int nq = (Wo + 3) >> 2;                                // quads of a row, the last one partial when Wo % 4 != 0
    const int y0 = blockIdx.x * a.rows, rows = min(a.rows, Ho - y0);
    uint8_t* out = dst + (size_t)b * 3 * oplane;

    for (int i = tid; i < nq * rows; i += AUG_THREADS) {
        const int ry = i / nq, q = i - ry * nq, y = y0 + ry, xq = 4 * q;
        int X0 = 0, Y0 = 0;
        if (WARP) {
            X0 = rn_i32((m1 * (double)y + m2) * 1024.0) + 16;
            Y0 = rn_i32((m4 * (double)y + m5) * 1024.0) + 16;
        }
        uint32_t w0 = 0, w1 = 0, w2 = 0;                         // the four pixels of planes R, G, B
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = xq + k;
            int r = 0, g = 0, bl = 0;
            if (x < Wo) {
                if (WARP) {
                    const int ad = rn_i32(m0 * (double)x * 1024.0), bd = rn_i32(m3 * (double)x * 1024.0);
                    // (unsigned sums: defined whatever a caller of the C entry hands in; an admitted call never wraps)
                    const int X = (int)((uint32_t)X0 + (uint32_t)ad) >> 5, Y = (int)((uint32_t)Y0 + (uint32_t)bd) >> 5;
                    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
                    int a0, a1, a2, b0, b1, b2, c0, c1, c2, d0, d1, d2;
                    canvas3(cv, src, W, plane, sy, sx, a0, a1, a2);
                    canvas3(cv, src, W, plane, sy, sx + 1, b0, b1, b2);
                    canvas3(cv, src, W, plane, sy + 1, sx, c0, c1, c2);
                    canvas3(cv, src, W, plane, sy + 1, sx + 1, d0, d1, d2);
                    const int wa = (32 - fx) * (32 - fy), wb = fx * (32 - fy), wc = (32 - fx) * fy, wd = fx * fy;
                    r = (wa * a0 + wb * b0 + wc * c0 + wd * d0 + 512) >> 10;
                    g = (wa * a1 + wb * b1 + wc * c1 + wd * d1 + 512) >> 10;
                    bl = (wa * a2 + wb * b2 + wc * c2 + wd * d2 + 512) >> 10;
                } else {
                    canvas3(cv, src, W, plane, y, x, r, g, bl);
                }
                if (jitter) hsv_jitter(lut, sdiv, hdiv, r, g, bl);
            }
            const int sh = 8 * (flip ? 3 - k : k);               // a flipped quad is stored byte-reversed
            w0 |= (uint32_t)r << sh;
            w1 |= (uint32_t)g << sh;
            w2 |= (uint32_t)bl << sh;
        }
        const size_t row = (size_t)y * Wo;
        if (a.vec4) {
            const size_t o = row + (flip ? Wo - 4 - xq : xq);
            *(uint32_t*)(out + o) = w0;
            *(uint32_t*)(out + oplane + o) = w1;
            *(uint32_t*)(out + 2 * oplane + o) = w2;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = xq + k;
                if (x < Wo) {
                    const size_t o = row + (flip ? Wo - 1 - x : x);
                    const int sh = 8 * (flip ? 3 - k : k);
                    out[o] = (uint8_t)(w0 >> sh);
                    out[oplane + o] = (uint8_t)(w1 >> sh);
                    out[2 * oplane + o] = (uint8_t)(w2 >> sh);
                }
            }
        }
    }
}

bool ranges_overlap(const uint8_t* p, size_t n, const uint8_t* q, size_t m) {
    return (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}

}  // namespace

extern "C" int dyk_augment_pairs_rows(const DykAugmentDesc* d, int32_t rows, void* stream) {
    if (rows < 1 || rows > 64) return DYK_ERR_ARG;
    if (!d || !d->src_v || !d->src_l || !d->dst_v || !d->dst_l) return DYK_ERR_ARG;
    if (d->N < 1 || d->B < 1 || d->H < 1 || d->W < 1 || d->Ho < 1 || d->Wo < 1) return DYK_ERR_ARG;
    if (d->N > AUG_MAX_SIZE || d->B > AUG_MAX_SIZE || d->H > AUG_MAX_SIZE || d->W > AUG_MAX_SIZE || d->Ho > AUG_MAX_SIZE ||
        d->Wo > AUG_MAX_SIZE)
        return DYK_ERR_ARG;
    if (d->rects && (d->Hc < 1 || d->Wc < 1 || d->Hc > AUG_MAX_SIZE || d->Wc > AUG_MAX_SIZE)) return DYK_ERR_ARG;
    if (!d->rects && d->B > d->N) return DYK_ERR_ARG;
    const int Hc = d->rects ? d->Hc : d->H, Wc = d->rects ? d->Wc : d->W;
    if (!d->minv && (d->Ho != Hc || d->Wo != Wc)) return DYK_ERR_ARG;
    const size_t sn = (size_t)d->N * 3 * d->H * d->W, dn = (size_t)d->B * 3 * d->Ho * d->Wo;
    const bool in_place_ok = !d->minv && !d->rects && !d->flip && d->B == d->N;
    const uint8_t* srcs[2] = {d->src_v, d->src_l};
    uint8_t* dsts[2] = {d->dst_v, d->dst_l};
    if (ranges_overlap(d->dst_v, dn, d->dst_l, dn)) return DYK_ERR_ARG;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            if (ranges_overlap(dsts[i], dn, srcs[j], sn) && !(in_place_ok && i == j && dsts[i] == srcs[j])) return DYK_ERR_ARG;

    AugArgs a;
    a.src[0] = d->src_v; a.src[1] = d->src_l; a.dst[0] = d->dst_v; a.dst[1] = d->dst_l;
    a.N = d->N; a.B = d->B; a.H = d->H; a.W = d->W; a.Hc = Hc; a.Wc = Wc; a.Ho = d->Ho; a.Wo = d->Wo;
    a.rects = d->rects; a.minv = d->minv; a.luts = d->luts; a.flip = d->flip;
    a.vec4 = d->Wo % 4 == 0 && (uintptr_t)d->dst_v % 4 == 0 && (uintptr_t)d->dst_l % 4 == 0;
    a.rows = rows;
    const dim3 grid((d->Ho + a.rows - 1) / a.rows, d->B, 2);
    if (d->minv) hipLaunchKernelGGL(augment_kernel<true>, grid, dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(augment_kernel<false>, grid, dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_augment_pairs(const DykAugmentDesc* d, void* stream) { return dyk_augment_pairs_rows(d, AUG_ROWS, stream); }
