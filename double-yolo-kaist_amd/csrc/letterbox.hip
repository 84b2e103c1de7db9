// dyk_resize_pad_pairs: resize (LINEAR / AREA) and letterbox of image pairs in one launch (reference build_utils/img_utils.py
// letterbox, the cv2.resize of kaist_dataset.py load_image, the BGR HWC -> RGB CHW of __getitem__).  The rule is stated once, in
// include/dyk_hip.h; tests/letterbox_ref.py restates it in plain numpy and the outputs are equal bit for bit.
//   grid   (bands of RP_ROWS = 8 output rows, B images, 2 streams); one workgroup owns a band of one output image of one stream
//   LDS    the source rows the band needs, whole rows, copied with 16-byte loads (the chunk keeps its global misalignment, so
//          only a head and a tail of at most 15 bytes go by bytes); in the interleaved layout one chunk serves the three
//          planes.  A band whose rows do not fit RP_STAGE bytes (a steep shrink of a wide image) reads its taps from global
//          memory instead: the same code over another base pointer.
//   thread four consecutive output columns of RP_ROWS / RP_GROUPS rows of all three planes: the column coefficients are
//          formed once per thread from the column index (no table in memory) and serve 12 quads; the row coefficients are
//          formed once per band row, in LDS.  One dword store per quad (byte stores when Wo % 4 != 0 or dst is unaligned)
// fp64 / fp32: every multiply and add of the rule is an operation of its own; the library is built with -ffp-contract=on, so
// contraction is switched off for this file by pragma (as in clahe.hip and augment.hip).
#include "dyk_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_ROWS = 8;                   // output rows of one workgroup
constexpr int RP_GROUPS = 2;                 // row groups of a band: a thread walks RP_ROWS / RP_GROUPS rows
constexpr int RP_STAGE = 32768;              // bytes of staged source rows (plus 6 x 16: misalignment and rounding of three chunks)
constexpr int RP_MAX_SIZE = 16384;

enum { MODE_COPY = 0, MODE_LINEAR = 1, MODE_AREA_INT = 2, MODE_AREA_W = 3 };

struct RpArgs {
    const DykResizePadRec* recs;
    uint8_t* dst[2];
    int B, Ho, Wo, layout;
    int vec4;                                // Wo % 4 == 0 and both dst bases 4-byte aligned: dword stores
    uint8_t color[4];
};

// the taps of one destination index along one axis.  LINEAR: s (before the clamp of the tap rows), c0, c1.  weighted AREA: the
// taps s, s+1, .., s+n-1; the first weighs wh when `head`, the last wt when `tail`, every other wm.
struct Axis {
    int s, n, head, tail;
    float wh, wm, wt;
    int c0, c1;
};

__device__ __forceinline__ double axis_scale(int n_src, int n_dst) {
    const double inv = (double)n_dst / (double)n_src;
    return 1.0 / inv;
}

__device__ __forceinline__ void linear_axis(int d, int n_src, double scale, bool edge_reset, Axis& a) {
    double t = (double)d + 0.5;
    t = t * scale;
    t = t - 0.5;
    float f = (float)t;
    const float fl = floorf(f);
    f = f - fl;
    int s = (int)fl;
    if (edge_reset) {
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= n_src - 1) { s = n_src - 1; f = 0.f; }
    }
    a.s = s;
    a.c0 = (int)rintf((1.f - f) * 2048.f);   // half to even
    a.c1 = (int)rintf(f * 2048.f);
}

__device__ __forceinline__ void area_axis(int d, int n_src, double scale, Axis& a) {
    const double f1 = (double)d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, (double)n_src - f1);
    int s1 = (int)ceil(f1);
    const int s2 = min((int)floor(f2), n_src - 1);
    s1 = min(s1, s2);
    a.head = (double)s1 - f1 > 1e-3;
    a.tail = f2 - (double)s2 > 1e-3;
    a.wh = (float)(((double)s1 - f1) / cell);
    a.wm = (float)(1.0 / cell);
    a.wt = (float)(fmin(fmin(f2 - (double)s2, 1.0), cell) / cell);
    a.s = a.head ? s1 - 1 : s1;
    a.n = a.head + (s2 - s1) + a.tail;
}

__device__ __forceinline__ float tap_weight(const Axis a, int k) {
    return (k == 0 && a.head) ? a.wh : ((k == a.n - 1 && a.tail) ? a.wt : a.wm);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ uint32_t sat_rint_u8(float v) {
    const float r = rintf(v);                // half to even
    return (uint32_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

// where the taps of one plane lie: element (row r, column x) is base[off + (r - r0) * rs + x * ps]
struct Planes {
    long long off0, off1, off2;              // of the three output planes
    int r0, r1, rs, ps;                      // r0..r1: the rows that are there (staged: the band's; otherwise 0..h-1)
};

template <int MODE>
__device__ __forceinline__ uint32_t pixel(const uint8_t* base, long long off, const Planes p, const Axis ay, const Axis ax, int dy, int dx, int h,
                                          int w, int kx, int ky) {
    auto S = [&](int r, int x) -> int {      // every tap bounded by the record's h and w
        return base[off + (long long)(clampi(r, p.r0, p.r1) - p.r0) * p.rs + (long long)clampi(x, 0, w - 1) * p.ps];
    };
    if (MODE == MODE_COPY) return (uint32_t)S(dy, dx);
    if (MODE == MODE_LINEAR) {
        const int y0 = clampi(ay.s, 0, h - 1), y1 = clampi(ay.s + 1, 0, h - 1);
        int D0, D1;
        if (ax.s + 1 >= w) {
            D0 = S(y0, ax.s) * 2048;
            D1 = S(y1, ax.s) * 2048;
        } else {
            D0 = S(y0, ax.s) * ax.c0 + S(y0, ax.s + 1) * ax.c1;
            D1 = S(y1, ax.s) * ax.c0 + S(y1, ax.s + 1) * ax.c1;
        }
        const int o = (((ay.c0 * (D0 >> 4)) >> 16) + ((ay.c1 * (D1 >> 4)) >> 16) + 2) >> 2;
        return (uint32_t)clampi(o, 0, 255);
    }
    if (MODE == MODE_AREA_INT) {
        int sum = 0;
        for (int j = 0; j < ky; ++j)
            for (int i = 0; i < kx; ++i) sum += S(dy * ky + j, dx * kx + i);
        if (kx == 2 && ky == 2) return (uint32_t)((sum + 2) >> 2);
        return sat_rint_u8((float)sum * (1.f / (float)(kx * ky)));
    }
    float acc = 0.f;
    for (int j = 0; j < ay.n; ++j) {
        const float beta = tap_weight(ay, j);
        float buf = 0.f;
        for (int i = 0; i < ax.n; ++i) buf = buf + (float)S(ay.s + j, ax.s + i) * tap_weight(ax, i);
        acc = j == 0 ? beta * buf : acc + beta * buf;
    }
    return sat_rint_u8(acc);
}

// the band [y0, y0 + rows) of one output image of one stream, taps read through `base` (LDS or the source itself)
template <int MODE>
__device__ __forceinline__ void band(const RpArgs& a, const DykResizePadRec& r, const uint8_t* base, const Planes& pl, const Axis* yrec,
                                     uint8_t* out, int y0, int rows, double scale_x, int kx, int ky) {
    const int Wo = a.Wo;
    const size_t oplane = (size_t)a.Ho * Wo;
    const int nq = (Wo + 3) >> 2;
    constexpr int GR = RP_ROWS / RP_GROUPS;
    for (int i = threadIdx.x; i < nq * RP_GROUPS; i += RP_THREADS) {
        const int g = i / nq, q = i - g * nq, xq = 4 * q;
        // the four columns' taps in named records (an array of them would live in scratch)
        Axis ax0, ax1, ax2, ax3;
        auto column = [&](int k, Axis& ax) -> bool {
            const int dx = xq + k - r.left;
            const bool in = dx >= 0 && dx < r.nw;
            ax = Axis{0, 0, 0, 0, 0.f, 0.f, 0.f, 0, 0};
            if (in && MODE == MODE_LINEAR) linear_axis(dx, r.w, scale_x, true, ax);
            if (in && MODE == MODE_AREA_W) area_axis(dx, r.w, scale_x, ax);
            return in;
        };
        const bool in0 = column(0, ax0), in1 = column(1, ax1), in2 = column(2, ax2), in3 = column(3, ax3);
        for (int ry = g * GR; ry < min(g * GR + GR, rows); ++ry) {
            const int y = y0 + ry, dy = y - r.top;
            const bool iny = dy >= 0 && dy < r.nh;
            const Axis ay = yrec[ry];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long long off = c == 0 ? pl.off0 : (c == 1 ? pl.off1 : pl.off2);
                auto px = [&](int k, bool in, const Axis ax) -> uint32_t {
                    if (!(iny && in)) return (uint32_t)a.color[c];
                    return pixel<MODE>(base, off, pl, ay, ax, dy, xq + k - r.left, r.h, r.w, kx, ky);
                };
                const uint32_t word = px(0, in0, ax0) | px(1, in1, ax1) << 8 | px(2, in2, ax2) << 16 | px(3, in3, ax3) << 24;
                uint8_t* o = out + c * oplane + (size_t)y * Wo + xq;
                if (a.vec4) {
                    *(uint32_t*)o = word;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (xq + k < Wo) o[k] = (uint8_t)(word >> (8 * k));
                }
            }
        }
    }
}

// n bytes g[0..n) -> d[0..n), d and g congruent mod 16: the middle with 16-byte loads, head and tail by bytes; reads only g[0..n)
__device__ __forceinline__ void stage_chunk(uint8_t* d, const uint8_t* g, int n) {
    const int tid = threadIdx.x;
    const int head = min(n, (int)((16 - ((uintptr_t)g & 15)) & 15));
    const int nvec = (n - head) >> 4;
    if (tid < head) d[tid] = g[tid];
    for (int i = tid; i < nvec; i += RP_THREADS) *(uint4*)(d + head + 16 * i) = *(const uint4*)(g + head + 16 * i);
    const int done = head + 16 * nvec;
    if (tid < n - done) d[done + tid] = g[done + tid];
}

__global__ __launch_bounds__(RP_THREADS) void resize_pad_kernel(const RpArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[RP_STAGE + 6 * 16];
    __shared__ Axis yrec[RP_ROWS];
    const int tid = threadIdx.x, b = blockIdx.y, stream = blockIdx.z;
    const DykResizePadRec r = a.recs[b];
    const uint8_t* src = stream == 0 ? r.src_v : r.src_l;
    uint8_t* out = (stream == 0 ? a.dst[0] : a.dst[1]) + (size_t)b * 3 * a.Ho * a.Wo;
    const int y0 = blockIdx.x * RP_ROWS, rows = min(RP_ROWS, a.Ho - y0);
    const int h = r.h, w = r.w;

    // the mode of this image (uniform over the workgroup)
    int mode, kx = 1, ky = 1;
    if (r.nh == h && r.nw == w) mode = MODE_COPY;
    else if (r.interp == 1 || (w == 2 * r.nw && h == 2 * r.nh)) {
        if (w % r.nw == 0 && h % r.nh == 0) { mode = MODE_AREA_INT; kx = w / r.nw; ky = h / r.nh; }
        else mode = MODE_AREA_W;
    } else mode = MODE_LINEAR;
    const double scale_x = axis_scale(w, r.nw), scale_y = axis_scale(h, r.nh);

    // the row taps of the band, once per row
    if (tid < RP_ROWS) {
        Axis ay = Axis{0, 0, 0, 0, 0.f, 0.f, 0.f, 0, 0};
        const int dy = y0 + tid - r.top;
        if (tid < rows && dy >= 0 && dy < r.nh) {
            if (mode == MODE_LINEAR) linear_axis(dy, h, scale_y, false, ay);
            if (mode == MODE_AREA_W) area_axis(dy, h, scale_y, ay);
        }
        yrec[tid] = ay;
    }
    __syncthreads();

    // the source rows [r_lo, r_hi] of the band's content rows [d_lo, d_hi]
    const int d_lo = max(y0 - r.top, 0), d_hi = min(y0 + rows - 1 - r.top, r.nh - 1);
    Planes pl;
    pl.rs = a.layout ? 3 * w : w;
    pl.ps = a.layout ? 3 : 1;
    bool staged = false;
    if (d_lo <= d_hi) {
        int r_lo, r_hi;
        const Axis lo = yrec[d_lo + r.top - y0], hi = yrec[d_hi + r.top - y0];
        if (mode == MODE_COPY) { r_lo = d_lo; r_hi = d_hi; }
        else if (mode == MODE_LINEAR) { r_lo = lo.s; r_hi = hi.s + 1; }
        else if (mode == MODE_AREA_INT) { r_lo = d_lo * ky; r_hi = d_hi * ky + ky - 1; }
        else { r_lo = lo.s; r_hi = hi.s + hi.n - 1; }
        r_lo = clampi(r_lo, 0, h - 1);
        r_hi = clampi(r_hi, r_lo, h - 1);
        const long long chunk = (long long)(r_hi - r_lo + 1) * pl.rs;                        // bytes of one contiguous chunk
        staged = chunk * (a.layout ? 1 : 3) <= RP_STAGE;
        if (staged) {
            pl.r0 = r_lo;
            pl.r1 = r_hi;
            if (a.layout) {
                const uint8_t* g = src + (size_t)r_lo * pl.rs;
                const int mis = (int)((uintptr_t)g & 15);
                stage_chunk(stage + mis, g, (int)chunk);
                pl.off0 = mis + 2; pl.off1 = mis + 1; pl.off2 = mis;
            } else {
                const int pitch = (((int)chunk + 15) & ~15) + 16;        // chunk c starts at c * pitch + its misalignment (< 16)
                const uint8_t* g0 = src + (size_t)r_lo * w;
                const uint8_t* g1 = g0 + (size_t)h * w;
                const uint8_t* g2 = g1 + (size_t)h * w;
                pl.off0 = (int)((uintptr_t)g0 & 15);
                pl.off1 = pitch + (int)((uintptr_t)g1 & 15);
                pl.off2 = 2 * pitch + (int)((uintptr_t)g2 & 15);
                stage_chunk(stage + pl.off0, g0, (int)chunk);
                stage_chunk(stage + pl.off1, g1, (int)chunk);
                stage_chunk(stage + pl.off2, g2, (int)chunk);
            }
            __syncthreads();
        }
    }
    if (!staged) {
        pl.r0 = 0;
        pl.r1 = h - 1;
        pl.off0 = a.layout ? 2 : 0;
        pl.off1 = a.layout ? 1 : (long long)h * w;
        pl.off2 = a.layout ? 0 : 2 * (long long)h * w;
    }

#define RP_BAND(M)                                                                     \
    if (staged) band<M>(a, r, stage, pl, yrec, out, y0, rows, scale_x, kx, ky);        \
    else band<M>(a, r, src, pl, yrec, out, y0, rows, scale_x, kx, ky)
    if (mode == MODE_COPY) { RP_BAND(MODE_COPY); }
    else if (mode == MODE_LINEAR) { RP_BAND(MODE_LINEAR); }
    else if (mode == MODE_AREA_INT) { RP_BAND(MODE_AREA_INT); }
    else { RP_BAND(MODE_AREA_W); }
#undef RP_BAND
}

bool ranges_overlap(const uint8_t* p, size_t n, const uint8_t* q, size_t m) {
    return (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}

}  // namespace

extern "C" int dyk_resize_pad_pairs(const DykResizePadDesc* d, void* stream) {
    if (!d || !d->recs || !d->recs_host || !d->dst_v || !d->dst_l) return DYK_ERR_ARG;
    if (d->B < 1 || d->Ho < 1 || d->Wo < 1) return DYK_ERR_ARG;
    if (d->B > RP_MAX_SIZE || d->Ho > RP_MAX_SIZE || d->Wo > RP_MAX_SIZE) return DYK_ERR_ARG;
    if (d->layout != 0 && d->layout != 1) return DYK_ERR_ARG;
    const size_t dn = (size_t)d->B * 3 * d->Ho * d->Wo;
    if (ranges_overlap(d->dst_v, dn, d->dst_l, dn)) return DYK_ERR_ARG;
    for (int b = 0; b < d->B; ++b) {
        const DykResizePadRec& r = d->recs_host[b];
        if (!r.src_v || !r.src_l) return DYK_ERR_ARG;
        if (r.h < 1 || r.w < 1 || r.nh < 1 || r.nw < 1) return DYK_ERR_ARG;
        if (r.h > RP_MAX_SIZE || r.w > RP_MAX_SIZE || r.nh > RP_MAX_SIZE || r.nw > RP_MAX_SIZE) return DYK_ERR_ARG;
        if (r.interp != 0 && r.interp != 1) return DYK_ERR_ARG;
        if (r.top < 0 || r.left < 0 || r.top > d->Ho - r.nh || r.left > d->Wo - r.nw) return DYK_ERR_ARG;
        if (r.interp == 1 && (r.nw > r.w || r.nh > r.h)) return DYK_ERR_ARG;
        const size_t sn = (size_t)3 * r.h * r.w;
        if (ranges_overlap(d->dst_v, dn, r.src_v, sn) || ranges_overlap(d->dst_v, dn, r.src_l, sn) ||
            ranges_overlap(d->dst_l, dn, r.src_v, sn) || ranges_overlap(d->dst_l, dn, r.src_l, sn))
            return DYK_ERR_ARG;
    }
    RpArgs a;
    a.recs = d->recs;
    a.dst[0] = d->dst_v; a.dst[1] = d->dst_l;
    a.B = d->B; a.Ho = d->Ho; a.Wo = d->Wo; a.layout = d->layout;
    a.vec4 = d->Wo % 4 == 0 && (uintptr_t)d->dst_v % 4 == 0 && (uintptr_t)d->dst_l % 4 == 0;
    a.color[0] = d->color[0]; a.color[1] = d->color[1]; a.color[2] = d->color[2]; a.color[3] = 0;
    const dim3 grid((d->Ho + RP_ROWS - 1) / RP_ROWS, d->B, 2);
    hipLaunchKernelGGL(resize_pad_kernel, grid, dim3(RP_THREADS), 0, (hipStream_t)stream, a);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
