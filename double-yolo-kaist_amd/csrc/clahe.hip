// dyk_clahe: OpenCV's 8-bit CLAHE per plane, and dyk_cutout_rects: the snowflake cut-outs (build_utils/snowflake.py).
// The rule is stated once, in include/dyk_hip.h; tests/clahe_ref.py restates it in plain numpy and the outputs are equal bit
// for bit.  Two launches:
//   clahe_table_kernel   one workgroup per (tile, plane): histogram -> clip -> redistribute -> prefix sum -> 256-entry table.
//                        All integer work up to the single fp32 multiply of the table entry, so no accumulation order shows.
//   clahe_interp_kernel  one workgroup per band of rows of a plane: the (at most three) tile rows of tables the band touches
//                        go to LDS, every source byte is read once and every result written once.
// fp32: every multiply and add of the rule is an operation of its own.  The library is built with -ffp-contract=on and the
// __fmul_rn / __fadd_rn / __fsub_rn of the HIP headers are plain `x * y`, `x + y`, `x - y`, so contraction is switched off for
// this file by pragma; the two reciprocals and lutScale are formed on the host and arrive as kernel arguments.
#include "dyk_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CLAHE_THREADS = 256;
constexpr int CLAHE_WAVES = CLAHE_THREADS / DYK_WAVE;
constexpr int CLAHE_BINS = 256;
constexpr int CLAHE_MAX_TILES = 16;          // per axis
constexpr int CLAHE_BAND_ROWS = 16;          // rows of one interpolation workgroup (never more than th: see clahe_geom)
constexpr int CLAHE_BAND_TROWS = 3;          // tile rows a band of <= th rows can touch

struct ClaheGeom {
    int planes, H, W, tiles_x, tiles_y;
    int tw, th;                              // tile size on the extended image
    int clip;                                // 0: no clipping
    int band;                                // rows per interpolation workgroup
    int vec4;                                // rows and bases are 4-byte aligned: uint32 loads and stores
    int lut16;                               // the workspace is 16-byte aligned: 16-byte copies of the tables to LDS
    float lut_scale, inv_tw, inv_th;
};

// index j of the image extended by BORDER_REFLECT_101 -> index into the n real ones
__device__ inline int reflect101(int j, int n) { return j < n ? j : 2 * (n - 1) - j; }

__device__ inline uint8_t sat_u8(float v) {
    const float r = rintf(v);                // v_rndne_f32: half to even
    return (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

// four pixels -> at most four LDS atomics, one per distinct value (a flat region costs one atomic per four pixels)
__device__ inline void hist_add4(int* h, uint32_t w) {
    const uint32_t v0 = w & 255u, v1 = (w >> 8) & 255u, v2 = (w >> 16) & 255u, v3 = w >> 24;
    atomicAdd(h + v0, 1 + (int)(v1 == v0) + (int)(v2 == v0) + (int)(v3 == v0));
    if (v1 != v0) atomicAdd(h + v1, 1 + (int)(v2 == v1) + (int)(v3 == v1));
    if (v2 != v0 && v2 != v1) atomicAdd(h + v2, 1 + (int)(v3 == v2));
    if (v3 != v0 && v3 != v1 && v3 != v2) atomicAdd(h + v3, 1);
}

__global__ __launch_bounds__(CLAHE_THREADS) void clahe_table_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ lut,
                                                                     const ClaheGeom g) {
    __shared__ int hist[CLAHE_WAVES][CLAHE_BINS];      // one histogram per wavefront: four waves do not meet on one hot bin
    __shared__ int wsum[CLAHE_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ntiles = g.tiles_x * g.tiles_y;
    const int tile = blockIdx.x % ntiles, plane = blockIdx.x / ntiles;
    const int tyi = tile / g.tiles_x, txi = tile % g.tiles_x;
    const uint8_t* p = src + (size_t)plane * g.H * g.W;
#pragma unroll
    for (int w = 0; w < CLAHE_WAVES; ++w) hist[w][tid] = 0;
    __syncthreads();

    int* h = hist[wave];
    const int x0 = txi * g.tw, y0 = tyi * g.th;
    // the 4-byte walk: whole words inside the real image (g.vec4 says rows and bases are aligned; tw % 4 keeps x0 on a word)
    const bool words = g.vec4 && (g.tw & 3) == 0 && x0 + g.tw <= g.W;
    if (words) {
        const int wq = g.tw >> 2, n = wq * g.th;
        for (int i = tid; i < n; i += CLAHE_THREADS) {
            const int y = i / wq, q = i - y * wq;
            const int ey = reflect101(y0 + y, g.H);
            hist_add4(h, *(const uint32_t*)(p + (size_t)ey * g.W + x0 + 4 * q));
        }
    } else {
        const int n = g.tw * g.th;
        for (int i = tid; i < n; i += CLAHE_THREADS) {
            const int y = i / g.tw, x = i - y * g.tw;
            const int ey = reflect101(y0 + y, g.H), ex = reflect101(x0 + x, g.W);
            atomicAdd(h + p[(size_t)ey * g.W + ex], 1);
        }
    }
    __syncthreads();

    // thread i owns bin i from here on
    int v = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
    if (g.clip > 0) {
        int over = v > g.clip ? v - g.clip : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) over += __shfl_xor(over, o, 64);
        if (lane == 0) wsum[wave] = over;
        __syncthreads();
        const int clipped = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();                                         // wsum is reused by the scan below
        const int batch = clipped / CLAHE_BINS, residual = clipped - batch * CLAHE_BINS;
        v = (v > g.clip ? g.clip : v) + batch;
        if (residual != 0) {
            // the reference's loop `for (i = 0; i < 256 && residual > 0; i += step, residual--) ++hist[i]` in closed form
            const int step = CLAHE_BINS / residual > 1 ? CLAHE_BINS / residual : 1;
            if (tid % step == 0 && tid / step < residual) v += 1;
        }
    }
    // inclusive prefix sum over the 256 bins: wave scan, then the totals of the waves in front
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(s, o, 64);
        if (lane >= o) s += t;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    for (int w = 0; w < wave; ++w) s += wsum[w];
    lut[((size_t)plane * ntiles + tile) * CLAHE_BINS + tid] = sat_u8(__fmul_rn((float)s, g.lut_scale));
}

// one pixel of the rule: the four table reads and the bilinear blend, every operation rounded on its own
__device__ inline uint8_t clahe_pixel(const uint8_t* __restrict__ l1, const uint8_t* __restrict__ l2, int x, uint32_t v,
                                      float ya, float ya1, const ClaheGeom& g) {
    const float txf = __fsub_rn(__fmul_rn((float)x, g.inv_tw), 0.5f);
    int tx1 = (int)floorf(txf);
    const float xa = __fsub_rn(txf, (float)tx1), xa1 = __fsub_rn(1.0f, xa);
    int tx2 = tx1 + 1;                                           // clamped after xa is formed
    tx1 = tx1 < 0 ? 0 : tx1;
    tx2 = tx2 > g.tiles_x - 1 ? g.tiles_x - 1 : tx2;
    const int i1 = tx1 * CLAHE_BINS + (int)v, i2 = tx2 * CLAHE_BINS + (int)v;
    const float top = __fadd_rn(__fmul_rn((float)l1[i1], xa1), __fmul_rn((float)l1[i2], xa));
    const float bot = __fadd_rn(__fmul_rn((float)l2[i1], xa1), __fmul_rn((float)l2[i2], xa));
    return sat_u8(__fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya)));
}

__global__ __launch_bounds__(CLAHE_THREADS) void clahe_interp_kernel(const uint8_t* src, uint8_t* dst,
                                                                      const uint8_t* __restrict__ lut, const ClaheGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[CLAHE_BAND_TROWS * CLAHE_MAX_TILES * CLAHE_BINS];
    const int tid = threadIdx.x;
    const int nbands = (g.H + g.band - 1) / g.band;
    const int band = blockIdx.x % nbands, plane = blockIdx.x / nbands;
    const int y0 = band * g.band, y1 = min(y0 + g.band, g.H);
    const int ntiles = g.tiles_x * g.tiles_y;
    // tile rows of the band: ty1 of its first row .. ty2 of its last, both clamped.  band <= th, so at most three.
    int ty_lo = (int)floorf(__fsub_rn(__fmul_rn((float)y0, g.inv_th), 0.5f));
    int ty_hi = (int)floorf(__fsub_rn(__fmul_rn((float)(y1 - 1), g.inv_th), 0.5f)) + 1;
    ty_lo = ty_lo < 0 ? 0 : ty_lo;
    ty_hi = ty_hi > g.tiles_y - 1 ? g.tiles_y - 1 : ty_hi;
    ty_hi = min(ty_hi, ty_lo + CLAHE_BAND_TROWS - 1);            // (never binds; keeps the copy inside `tab` whatever the input)
    const int row_bytes = g.tiles_x * CLAHE_BINS;                // a multiple of 256: 16-byte copies
    {
        const uint8_t* s = lut + ((size_t)plane * ntiles + (size_t)ty_lo * g.tiles_x) * CLAHE_BINS;
        const int nbytes = (ty_hi - ty_lo + 1) * row_bytes;
        if (g.lut16) {
            for (int i = tid; i < nbytes / 16; i += CLAHE_THREADS) ((uint4*)tab)[i] = ((const uint4*)s)[i];
        } else {
            for (int i = tid; i < nbytes; i += CLAHE_THREADS) tab[i] = s[i];
        }
    }
    __syncthreads();

    const size_t base = (size_t)plane * g.H * g.W;
    const int rows = y1 - y0;
    if (g.vec4) {
        const int wq = g.W >> 2, n = wq * rows;
        for (int i = tid; i < n; i += CLAHE_THREADS) {
            const int r = i / wq, q = i - r * wq, y = y0 + r;
            const float tyf = __fsub_rn(__fmul_rn((float)y, g.inv_th), 0.5f);
            int ty1 = (int)floorf(tyf);
            const float ya = __fsub_rn(tyf, (float)ty1), ya1 = __fsub_rn(1.0f, ya);
            int ty2 = ty1 + 1;
            ty1 = ty1 < 0 ? 0 : ty1;
            ty2 = ty2 > g.tiles_y - 1 ? g.tiles_y - 1 : ty2;
            const uint8_t* l1 = tab + min(ty1 - ty_lo, CLAHE_BAND_TROWS - 1) * row_bytes;
            const uint8_t* l2 = tab + min(ty2 - ty_lo, CLAHE_BAND_TROWS - 1) * row_bytes;
            const size_t off = base + (size_t)y * g.W + 4 * q;
            const uint32_t w = *(const uint32_t*)(src + off);
            uint32_t o = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                o |= (uint32_t)clahe_pixel(l1, l2, 4 * q + k, (w >> (8 * k)) & 255u, ya, ya1, g) << (8 * k);
            *(uint32_t*)(dst + off) = o;
        }
    } else {
        const int n = g.W * rows;
        for (int i = tid; i < n; i += CLAHE_THREADS) {
            const int r = i / g.W, x = i - r * g.W, y = y0 + r;
            const float tyf = __fsub_rn(__fmul_rn((float)y, g.inv_th), 0.5f);
            int ty1 = (int)floorf(tyf);
            const float ya = __fsub_rn(tyf, (float)ty1), ya1 = __fsub_rn(1.0f, ya);
            int ty2 = ty1 + 1;
            ty1 = ty1 < 0 ? 0 : ty1;
            ty2 = ty2 > g.tiles_y - 1 ? g.tiles_y - 1 : ty2;
            const size_t off = base + (size_t)y * g.W + x;
            const uint8_t* l1 = tab + min(ty1 - ty_lo, CLAHE_BAND_TROWS - 1) * row_bytes;
            const uint8_t* l2 = tab + min(ty2 - ty_lo, CLAHE_BAND_TROWS - 1) * row_bytes;
            dst[off] = clahe_pixel(l1, l2, x, src[off], ya, ya1, g);
        }
    }
}

// geometry and constants of the rule, or false for the refused arguments
bool clahe_geom(const DykClaheDesc* d, ClaheGeom& g) {
    if (!d || !d->src || !d->dst || !d->lut) return false;
    if (d->planes < 1 || d->H < 1 || d->W < 1) return false;
    if (d->tiles_x < 1 || d->tiles_x > CLAHE_MAX_TILES || d->tiles_y < 1 || d->tiles_y > CLAHE_MAX_TILES) return false;
    int padx = 0, pady = 0;
    if (d->W % d->tiles_x != 0 || d->H % d->tiles_y != 0) {
        padx = d->tiles_x - d->W % d->tiles_x;                   // a divisible axis gets a full extra tiles_x: OpenCV's behaviour
        pady = d->tiles_y - d->H % d->tiles_y;
    }
    if (padx > d->W - 1 || pady > d->H - 1) return false;        // the reflection 2(n-1) - j would leave the image
    g.planes = d->planes; g.H = d->H; g.W = d->W; g.tiles_x = d->tiles_x; g.tiles_y = d->tiles_y;
    g.tw = (d->W + padx) / d->tiles_x;
    g.th = (d->H + pady) / d->tiles_y;
    const int64_t area = (int64_t)g.tw * g.th;
    if (area > (1 << 24)) return false;                          // float(prefix sum) must be exact
    const int64_t per_plane = d->H > 256 ? d->H : 256;           // workgroups of a plane: <= 256 tiles, <= H bands
    if ((int64_t)d->planes * per_plane > 2147483647LL) return false;                 // one grid dimension
    g.lut_scale = 255.0f / (float)area;
    g.clip = 0;
    if (d->clip_limit > 0) {
        const double c = d->clip_limit * (double)area / 256.0;
        g.clip = c >= 2147483647.0 ? 2147483647 : (int)c;
        if (g.clip < 1) g.clip = 1;
    }
    g.inv_tw = 1.0f / (float)g.tw;
    g.inv_th = 1.0f / (float)g.th;
    g.band = g.th < CLAHE_BAND_ROWS ? g.th : CLAHE_BAND_ROWS;
    g.lut16 = (uintptr_t)d->lut % 16 == 0;
    g.vec4 = (d->W % 4 == 0) && ((uintptr_t)d->src % 4 == 0) && ((uintptr_t)d->dst % 4 == 0);
    return true;
}

__global__ __launch_bounds__(CLAHE_THREADS) void cutout_rects_kernel(uint8_t* img, const int32_t* __restrict__ rects, int H,
                                                                      int W, int nrect, int planes_per_set, uint8_t value) {
    const int plane = blockIdx.x / nrect, r = blockIdx.x % nrect;
    const int32_t* q = rects + ((size_t)(plane / planes_per_set) * nrect + r) * 4;
    const int x0 = max(q[0], 0), y0 = max(q[1], 0), x1 = min(q[2], W), y1 = min(q[3], H);     // upper ends exclusive
    if (x1 <= x0 || y1 <= y0) return;                            // empty, inverted or outside: nothing is written
    const int rw = x1 - x0, n = rw * (y1 - y0);                  // <= H * W, which the host keeps inside int32
    uint8_t* p = img + (size_t)plane * H * W;
    for (int i = threadIdx.x; i < n; i += CLAHE_THREADS) {
        const int y = i / rw, x = i - y * rw;
        p[(size_t)(y0 + y) * W + x0 + x] = value;
    }
}

}  // namespace

extern "C" int64_t dyk_clahe_ws_bytes(int32_t planes, int32_t tiles_x, int32_t tiles_y) {
    if (planes < 1 || tiles_x < 1 || tiles_x > CLAHE_MAX_TILES || tiles_y < 1 || tiles_y > CLAHE_MAX_TILES) return DYK_ERR_ARG;
    return (int64_t)planes * tiles_x * tiles_y * CLAHE_BINS;
}

extern "C" int dyk_clahe(const DykClaheDesc* d, void* stream) {
    ClaheGeom g;
    if (!clahe_geom(d, g)) return DYK_ERR_ARG;
    const int ntiles = g.tiles_x * g.tiles_y, nbands = (g.H + g.band - 1) / g.band;
    hipLaunchKernelGGL(clahe_table_kernel, dim3(ntiles * g.planes), dim3(CLAHE_THREADS), 0, (hipStream_t)stream, d->src, d->lut, g);
    DYK_LAUNCH_CHECK();
    hipLaunchKernelGGL(clahe_interp_kernel, dim3(nbands * g.planes), dim3(CLAHE_THREADS), 0, (hipStream_t)stream, d->src, d->dst,
                       (const uint8_t*)d->lut, g);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_cutout_rects(uint8_t* img, int32_t planes, int32_t H, int32_t W, const int32_t* rects, int32_t nrect,
                                int32_t planes_per_set, int32_t value, void* stream) {
    if (!img || planes < 1 || H < 1 || W < 1 || nrect < 0 || planes_per_set < 1 || value < 0 || value > 255) return DYK_ERR_ARG;
    if ((int64_t)H * W > 2147483647LL || (int64_t)planes * (nrect > 0 ? nrect : 1) > 2147483647LL) return DYK_ERR_ARG;
    if (nrect == 0) return DYK_OK;
    if (!rects) return DYK_ERR_ARG;
    hipLaunchKernelGGL(cutout_rects_kernel, dim3(planes * nrect), dim3(CLAHE_THREADS), 0, (hipStream_t)stream, img, rects, H, W, nrect,
                       planes_per_set, (uint8_t)value);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
