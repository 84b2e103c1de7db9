// Depthwise convolution (groups == channels), forward / data gradient / weight gradient, channels-last.
// Replaces nn.Conv2d(groups=C) at reference models.py:41 (MobileNet [convolutional] sections with `groups=`)
// and the first conv of DepthwiseSeparableConv2d (layers.py:223-224).  4.5-12 flop/byte: HBM-bound, so these
// are streaming kernels (16-byte vectors of 8 channels, the k*k re-reads of a pixel neighbourhood come from
// L1/L2), not MFMA work.  Weights are read directly from the fp32 master copy in tap-major order [k*k][C].
// The forward optionally accumulates the per-channel sum / sum of squares for a following train-mode
// BatchNorm into the same replicated fp64 buffers the MFMA conv epilogue uses.
//
// Layout of this file: the tile constants; the five kernels; ONE tile geometry (dw_tile_geometry) for both LDS-tiled
// kernels; ONE route per op (dw_route_fwd / dw_route_dgrad / dw_route_wgrad) that maps a checked descriptor to a return code
// or a kernel choice with its launch parameters; the extern "C" entries, each check -> route -> launch.
// The order in which a route tests its refusals is observable (which code a doubly wrong descriptor gets) and is kept as it
// was; so is what dyk_dwconv_wgrad_rows answers for an even k -- the row kernel's plane count, although dyk_dwconv_wgrad then
// refuses the launch (no instantiation) -- see dw_route_wgrad.  tests/golden/dwconv_queries.json pins both.
// Device helpers: dw_load_f32 (the fp32 weight-vector load of every kernel) and dw_clamp are shared.  The role view of GRAD, the
// accumulate-and-store, the staging slot split, the `pre` activation, the BatchNorm vector load of the tiled data gradient and
// the weight-gradient lane fold are written out in each kernel ON PURPOSE: as shared helpers each of them changed the
// instructions of a kernel (order and register allocation, +0..30 instructions), and the probe cannot tell such a change from
// its own run-to-run spread.  Written out, the ten tiled instantiations compile to the instructions of the version
// before this layout, the other fifteen to the same instructions with a few of the prologue reordered.
#include <type_traits>
#include "dyk_common.h"

namespace {

// ---------------------------------------------------------------------------------------------- device helpers and tile constants
// EPV (4 | 8) consecutive floats from a 16-byte aligned address (global or LDS) as float4 loads
template <int EPV>
__device__ inline void dw_load_f32(const float* p, float* out) {
#pragma unroll
    for (int j = 0; j < EPV; j += 4) {
        const float4 q = *(const float4*)(p + j);
        out[j] = q.x; out[j + 1] = q.y; out[j + 2] = q.z; out[j + 3] = q.w;
    }
}

__device__ inline int dw_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ---- the LDS-tiled kernels' geometry.  Compile-time part: output tiles are TH x DW_TW pixels for CT <= 8 channel vectors, a
// thread owns a strip of DW_XT pixels; the (TH + K - 1) x (DW_TW + K - 1) patch is staged with dw_patch_loads(K) 16-byte loads
// per thread.  The kernels get CT and derive the rest with the functions dw_tile_geometry (host) uses.
constexpr int DW_TW = 16, DW_XT = 4, DW_SPR = DW_TW / DW_XT;
constexpr int dw_patch_loads(int k) { return k == 5 ? 8 : 6; }
__host__ __device__ inline int dw_tile_rows(int CT) { return (256 / CT) / DW_SPR; }     // TH: thread = (vector, strip, row)
__host__ __device__ inline int dw_slot_stride(int CT) { return CT | 1; }                // odd: <= 2-way bank conflicts

// ---------------------------------------------------------------------------------------------- kernels
// thread mapping: tx = channel vector in a group of CVB, ty = pixel lane; grid.x over channel-vector
// groups, grid.y strides over output pixels
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void dwconv_kernel(DykDwDesc d, int CVB) {
    constexpr int EPV = ElemTraits<T>::EPV;
    __shared__ float red[256 * 2 * 8];
    const int PY = 256 / CVB;
    const int tx = threadIdx.x % CVB, ty = threadIdx.x / CVB;
    const int cv = blockIdx.x * CVB + tx;
    const int c = cv * EPV;
    const bool active = c < d.C;
    const T* __restrict__ x = GRAD ? (const T*)d.y : (const T*)d.x;     // tensor read
    T* __restrict__ y = GRAD ? (T*)d.x : (T*)d.y;                       // tensor written
    const int ld_src = GRAD ? d.ldy : d.ldx, ld_dst = GRAD ? d.ldx : d.ldy;
    const int Hout = GRAD ? d.Hi : d.Ho, Wout = GRAD ? d.Wi : d.Wo;
    const int Hsrc = GRAD ? d.Ho : d.Hi, Wsrc = GRAD ? d.Wo : d.Wi;
    const int k = d.k, s = d.stride, pad = d.pad;
    // GRAD: dx[yi] += dy[(yi + pad - kh)/s] * w[kh] when divisible
    const bool accum = d.flags & DYK_EW_ACCUM;
    const bool stats = (!GRAD) && d.stats != nullptr;
    float s1[EPV], s2[EPV];
#pragma unroll
    for (int j = 0; j < EPV; ++j) s1[j] = s2[j] = 0.f;
    if (active) {
        // image rows over grid.y, pixels of a row over the pixel lanes: no per-pixel integer division
        const int nrows = d.B * Hout;
        for (int row = blockIdx.y; row < nrows; row += gridDim.y) {
          const int b = row / Hout, yo = row - b * Hout;
          for (int xo = ty; xo < Wout; xo += PY) {
            const long p = (long)row * Wout + xo;
            float acc[EPV];
#pragma unroll
            for (int j = 0; j < EPV; ++j) acc[j] = 0.f;
            for (int kh = 0; kh < k; ++kh) {
                int ys;
                if (GRAD) {
                    const int t = yo + pad - kh;
                    if (t < 0 || t % s) continue;
                    ys = t / s;
                } else {
                    ys = yo * s + kh - pad;
                }
                if (ys < 0 || ys >= Hsrc) continue;
                for (int kw = 0; kw < k; ++kw) {
                    int xs;
                    if (GRAD) {
                        const int t = xo + pad - kw;
                        if (t < 0 || t % s) continue;
                        xs = t / s;
                    } else {
                        xs = xo * s + kw - pad;
                    }
                    if (xs < 0 || xs >= Wsrc) continue;
                    float xv[EPV], wv[EPV];
                    vec_unpack<T>(*(const uint4*)(x + (((long)b * Hsrc + ys) * Wsrc + xs) * ld_src + c), xv);
                    dw_load_f32<EPV>(d.w + (long)(kh * k + kw) * d.C + c, wv);
#pragma unroll
                    for (int j = 0; j < EPV; ++j) acc[j] += xv[j] * wv[j];
                }
            }
            if (stats) {
#pragma unroll
                for (int j = 0; j < EPV; ++j) { s1[j] += acc[j]; s2[j] += acc[j] * acc[j]; }
            }
            T* yp = y + p * ld_dst + c;
            if (accum) {
                float old[EPV];
                vec_unpack<T>(*(const uint4*)yp, old);
#pragma unroll
                for (int j = 0; j < EPV; ++j) acc[j] += old[j];
            }
            *(uint4*)yp = vec_pack<T>(acc);
          }
        }
    }
    if (stats) {
        // fold of the pixel lanes through LDS in lane order, then one fp64 atomic per (channel, sum) onto this workgroup row's replica
        float* mine = red + threadIdx.x * 16;
#pragma unroll
        for (int j = 0; j < EPV; ++j) { mine[j] = s1[j]; mine[8 + j] = s2[j]; }
        __syncthreads();
        if (ty == 0 && active) {
            for (int q = 1; q < PY; ++q) {
                const float* o = red + (q * CVB + tx) * 16;
#pragma unroll
                for (int j = 0; j < EPV; ++j) { s1[j] += o[j]; s2[j] += o[8 + j]; }
            }
            double* st = d.stats + (size_t)(blockIdx.y % (unsigned)(d.stats_slots > 0 ? d.stats_slots : 1)) * 2 * d.C;
#pragma unroll
            for (int j = 0; j < EPV; ++j) {
                atomicAdd(st + c + j, (double)s1[j]);
                atomicAdd(st + d.C + c + j, (double)s2[j]);
            }
        }
    }
}

// LDS-tiled stride-1 depthwise conv (bf16 | fp16; forward, and the data gradient as the same correlation with the flipped kernel
// and pad' = K - 1 - pad).  A workgroup stages the input patch of a TH x 16 pixel output tile for CT <= 8 channel vectors
// in LDS -- every thread issues all of its (<= 8) 16-byte loads before anything waits, ONE memory round trip per tile
// -- and the k x k taps are then ds_read_b128s.  (Its predecessor, a register-strip kernel that re-read the patch through
// L1 in K dependent batches per strip, ran at 1.1-1.9 TB/s on the MobileNetV3 layers, latency-bound; it was removed once no
// shape could reach it, see dw_tile_geometry.)
// Thread = (channel vector ct, strip of XT = 4 pixels, tile row); tile [rows][cols][S = CT|1] 16-byte slots (odd slot
// stride: <= 2-way bank conflicts, irrelevant next to the VALU work); weights [K*K][CT*8] fp32 behind the tile.
template <int K, bool GRAD, typename T = bf16_t>
__global__ __launch_bounds__(256) void dwconv_tile_kernel(DykDwDesc d, int CT, int groups, unsigned m_ct, int tiles_x,
                                                          int tiles_y) {
    static_assert(sizeof(T) == 2, "16-bit elements (bf16 | f16)");
    constexpr int EPV = 8, TW = DW_TW, XT = DW_XT, SPR = DW_SPR, NS = XT + K - 1, IC = TW + K - 1;
    constexpr int NLD = dw_patch_loads(K);                     // staging loads per thread (dw_tile_geometry checks the tile fits)
    extern __shared__ uint4 smem[];
    const int S = dw_slot_stride(CT);
    const int RT = dw_tile_rows(CT), TH = RT, IR = TH + K - 1;
    float* wl = (float*)(smem + IR * IC * S);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int grp = bid % groups; bid /= groups;
    const int txi = bid % tiles_x; bid /= tiles_x;
    const int tyi = bid % tiles_y;
    const int b = bid / tiles_y;
    const int tile_id = (b * tiles_y + tyi) * tiles_x + txi;
    const int cv0 = grp * CT, CV = d.C / EPV;
    const T* __restrict__ x = GRAD ? (const T*)d.y : (const T*)d.x;     // tensor read
    T* __restrict__ y = GRAD ? (T*)d.x : (T*)d.y;                       // tensor written
    const int ld_src = GRAD ? d.ldy : d.ldx, ld_dst = GRAD ? d.ldx : d.ldy;
    const int Hout = GRAD ? d.Hi : d.Ho, Wout = GRAD ? d.Wi : d.Wo;
    const int Hsrc = GRAD ? d.Ho : d.Hi, Wsrc = GRAD ? d.Wo : d.Wi;
    const int padp = GRAD ? K - 1 - d.pad : d.pad;
    const int y0 = tyi * TH, x0 = txi * TW;
    const int tid = threadIdx.x;
    {   // ---- stage the patch: all loads first (clamped addresses), then the LDS stores (zeros outside the image)
        const int nvec = IR * IC * CT;
        uint4 u4[NLD];
        int dst[NLD], cts[NLD];
        unsigned okm = 0;
        const T* img = x + (long)b * Hsrc * Wsrc * ld_src + (long)cv0 * EPV;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const unsigned idx = tid + i * 256;
            const unsigned q = CT == 1 ? idx : __umulhi(idx, m_ct);     // idx / CT
            const int ct = (int)(idx - q * CT);
            const int row = (int)(q / IC), col = (int)(q - (unsigned)row * IC);
            const int ys = y0 + row - padp, xs = x0 + col - padp;
            const bool ok = idx < (unsigned)nvec && ys >= 0 && ys < Hsrc && xs >= 0 && xs < Wsrc && cv0 + ct < CV;
            const int cc = cv0 + ct < CV ? ct : 0;
            u4[i] = *(const uint4*)(img + ((long)dw_clamp(ys, Hsrc) * Wsrc + dw_clamp(xs, Wsrc)) * ld_src + cc * EPV);
            okm |= ok ? (1u << i) : 0u;
            cts[i] = cc;
            dst[i] = idx < (unsigned)nvec ? (row * IC + col) * S + ct : -1;
        }
        // weights of this channel group, tap order flipped for the data gradient
        for (int i = tid; i < K * K * CT * 2; i += 256) {
            const int tap = i / (CT * 2), rem = i - tap * (CT * 2);
            const int cch = cv0 * EPV + rem * 4;
            const int tsrc = GRAD ? K * K - 1 - tap : tap;
            float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cch < d.C) w4 = *(const float4*)(d.w + (long)tsrc * d.C + cch);
            *(float4*)(wl + (tap * CT * 2 + rem) * 4) = w4;
        }
        if (!GRAD && d.pre != nullptr) {
            // DykDwDesc.pre: the patch holds the RAW output of the expansion conv; z = dtype(act(scale * u + shift)) is formed
            // here, between the loads (all in flight) and the LDS stores.  scale | shift of this workgroup's channel vectors
            // go through LDS (behind the weights): a staged vector belongs to any of the CT vectors
            float* pl = wl + K * K * CT * 8;
            for (int i = tid; i < CT * 4; i += 256) {                 // i = (which, ct, half)
                const int which = i / (CT * 2), rem = i - which * (CT * 2);
                const int cch = cv0 * EPV + rem * 4;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (cch < d.C) q = *(const float4*)(d.pre + (long)which * d.C + cch);
                *(float4*)(pl + i * 4) = q;
            }
            __syncthreads();
            // (ONE switch around the whole pass: with the activation switch inside the unrolled loops the transform is all branches)
            auto xform = [&](auto act_tag) {
                constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
                for (int i = 0; i < NLD; ++i) {
                    float u[EPV], sc[EPV], sh[EPV];
                    vec_unpack<T>(u4[i], u);
                    dw_load_f32<EPV>(pl + cts[i] * 8, sc);
                    dw_load_f32<EPV>(pl + CT * 8 + cts[i] * 8, sh);
#pragma unroll
                    for (int j = 0; j < EPV; ++j) u[j] = act_fwd_c<ACT>(u[j] * sc[j] + sh[j], d.pre_act);
                    u4[i] = vec_pack<T>(u);
                }
            };
            switch (d.pre_act) {
            case DYK_ACT_RELU: xform(std::integral_constant<int, DYK_ACT_RELU>{}); break;
            case DYK_ACT_RELU6: xform(std::integral_constant<int, DYK_ACT_RELU6>{}); break;
            case DYK_ACT_HSWISH: xform(std::integral_constant<int, DYK_ACT_HSWISH>{}); break;
            case DYK_ACT_LEAKY: xform(std::integral_constant<int, DYK_ACT_LEAKY>{}); break;
            default: xform(std::integral_constant<int, -1>{}); break;
            }
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            if (!((okm >> i) & 1u)) u4[i] = make_uint4(0u, 0u, 0u, 0u);
            if (dst[i] >= 0) smem[dst[i]] = u4[i];
        }
    }
    __syncthreads();
    const unsigned sl = CT == 1 ? (unsigned)tid : __umulhi((unsigned)tid, m_ct);
    const int ct = tid - (int)sl * CT;
    const int strip = sl % SPR, r = sl / SPR;
    const bool active = r < RT && cv0 + ct < CV;
    const bool accum = d.flags & DYK_EW_ACCUM;
    const bool bnbwd = GRAD && d.res != nullptr;               // fused BatchNorm-backward reduce of the producer of x
    const bool stats = ((!GRAD) && d.stats != nullptr) || bnbwd;
    float s1[EPV], s2[EPV];
#pragma unroll
    for (int j = 0; j < EPV; ++j) s1[j] = s2[j] = 0.f;
    if (active) {
        float acc[XT][EPV];
#pragma unroll
        for (int o = 0; o < XT; ++o)
#pragma unroll
            for (int j = 0; j < EPV; ++j) acc[o][j] = 0.f;
        // the producer's raw conv output at this thread's four pixels: requested now, needed after the tap loop
        uint4 uraw[XT];
        float bsc[EPV], bsh[EPV], bmu[EPV], brs[EPV];
        if (GRAD && bnbwd) {
            const int c = (cv0 + ct) * EPV;
#pragma unroll
            for (int j = 0; j < EPV; j += 4) {
                const float4 q0 = *(const float4*)(d.bn + c + j), q1 = *(const float4*)(d.bn + d.C + c + j);
                const float4 q2 = *(const float4*)(d.bn + 2 * d.C + c + j), q3 = *(const float4*)(d.bn + 3 * d.C + c + j);
                bsc[j] = q0.x; bsc[j + 1] = q0.y; bsc[j + 2] = q0.z; bsc[j + 3] = q0.w;
                bsh[j] = q1.x; bsh[j + 1] = q1.y; bsh[j + 2] = q1.z; bsh[j + 3] = q1.w;
                bmu[j] = q2.x; bmu[j + 1] = q2.y; bmu[j + 2] = q2.z; bmu[j + 3] = q2.w;
                brs[j] = q3.x; brs[j + 1] = q3.y; brs[j + 2] = q3.z; brs[j + 3] = q3.w;
            }
            const int yo = y0 + r < Hout ? y0 + r : Hout - 1;
#pragma unroll
            for (int o = 0; o < XT; ++o) {
                const int xo = x0 + strip * XT + o;
                uraw[o] = *(const uint4*)((const T*)d.res + (((long)b * Hout + yo) * Wout + (xo < Wout ? xo : Wout - 1)) * d.ldr +
                                          (long)(cv0 + ct) * EPV);
            }
        }
        // (kernel rows NOT unrolled: hoisted together their LDS reads need 500 VGPRs -- one wave per SIMD)
#pragma unroll 1
        for (int kh = 0; kh < K; ++kh) {
            float wv[K][EPV];
#pragma unroll
            for (int kw = 0; kw < K; ++kw) dw_load_f32<EPV>(wl + ((kh * K + kw) * CT + ct) * 8, wv[kw]);
            const uint4* prow = smem + ((r + kh) * IC + strip * XT) * S + ct;
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                float xv[EPV];
                vec_unpack<T>(prow[q * S], xv);
#pragma unroll
                for (int o = 0; o < XT; ++o) {
                    const int kw = q - o;                          // compile-time after unrolling
                    if (kw < 0 || kw >= K) continue;
#pragma unroll
                    for (int j = 0; j < EPV; ++j) acc[o][j] += xv[j] * wv[kw][j];
                }
            }
        }
        const int yo = y0 + r;
        if (yo < Hout) {
#pragma unroll
            for (int o = 0; o < XT; ++o) {
                const int xo = x0 + strip * XT + o;
                if (xo >= Wout) break;
                if (GRAD && bnbwd) {
                    float u[EPV];
                    vec_unpack<T>(uraw[o], u);
                    // the gradient is rounded to the storage dtype first (what an unfused reduce pass would read back)
                    const uint4 pk = vec_pack<T>(acc[o]);
                    vec_unpack<T>(pk, acc[o]);
#pragma unroll
                    for (int j = 0; j < EPV; ++j) {
                        const float da = acc[o][j] * act_bwd(d.act, u[j] * bsc[j] + bsh[j]);
                        s1[j] += da;
                        s2[j] += da * ((u[j] - bmu[j]) * brs[j]);
                        acc[o][j] = da;
                    }
                } else if (stats) {
#pragma unroll
                    for (int j = 0; j < EPV; ++j) { s1[j] += acc[o][j]; s2[j] += acc[o][j] * acc[o][j]; }
                }
                T* yp = y + (((long)b * Hout + yo) * Wout + xo) * ld_dst + (long)(cv0 + ct) * EPV;
                if (accum) {
                    float old[EPV];
                    vec_unpack<T>(*(const uint4*)yp, old);
#pragma unroll
                    for (int j = 0; j < EPV; ++j) acc[o][j] += old[j];
                }
                *(uint4*)yp = vec_pack<T>(acc[o]);
            }
        }
    }
    if (stats) {
        // workgroup reduction in a fixed order (same sums from run to run), spread over all threads: thread (part, ct, j)
        // adds every parts-th strip lane of output (ct, j), the first 16 * CT threads fold the parts and issue ONE
        // fp64 atomic each -- eight threads walking 32 lanes and issuing 16 atomics apiece cost ~25 us per launch
        __syncthreads();                                       // everyone is done with the patch: reuse it
        float* red = (float*)smem;
        float* red2 = red + 256 * 16;
        float* mine = red + tid * 16;
#pragma unroll
        for (int j = 0; j < EPV; ++j) { mine[j] = s1[j]; mine[8 + j] = s2[j]; }
        __syncthreads();
        const int nout = 16 * CT, parts = 256 / nout, nsl = 256 / CT;
        const int part = tid / nout, o = tid - part * nout;
        if (part < parts) {
            float t = 0.f;
            for (int q = part; q < nsl; q += parts) t += red[q * nout + o];
            red2[part * nout + o] = t;
        }
        __syncthreads();
        if (tid < nout) {
            float t = 0.f;
            for (int p = 0; p < parts; ++p) t += red2[p * nout + tid];
            const int cto = tid >> 4, j = tid & 15;
            if (cv0 + cto < CV) {
                double* st = d.stats + (size_t)((unsigned)tile_id % (unsigned)(d.stats_slots > 0 ? d.stats_slots : 1)) * 2 * d.C;
                atomicAdd(st + (j < 8 ? 0 : d.C) + (cv0 + cto) * EPV + (j & 7), (double)t);
            }
        }
    }
}

// Stride-2 data gradient (MobileNet down-sampling layers): K and the stride are compile-time, so the taps of a pixel are a
// fixed, unrolled set whose loads are issued together -- clamped coordinates, values zeroed afterwards (dwconv_kernel
// walks runtime loops with a branch around every load: one memory round trip per tap).
//   dx[yi, xi] = sum over the taps of yi's / xi's parity, kh = (yi + pad) % 2 + 2 a:
//                dy[(yi + pad - kh) / 2, (xi + pad - kw) / 2] w[kh, kw]                              (ceil(K/2)^2 loads)
// (The stride-2 FORWARD runs on dwconv_kernel, which measured faster than the forward form this kernel once had.)
template <int K, typename T>
__global__ __launch_bounds__(256) void dwconv_s2_dgrad_kernel(DykDwDesc d, int CVB) {
    constexpr int EPV = ElemTraits<T>::EPV;
    constexpr int KT = (K + 1) / 2;                            // taps per dimension a pixel touches
    const int PY = 256 / CVB;
    const int tx = threadIdx.x % CVB, ty = threadIdx.x / CVB;
    const int c = (blockIdx.x * CVB + tx) * EPV;
    const T* __restrict__ dy = (const T*)d.y;                  // read: output gradient [B, Ho, Wo, C]
    T* __restrict__ dx = (T*)d.x;                              // written: input gradient [B, Hi, Wi, C]
    const int pad = d.pad;
    const bool accum = d.flags & DYK_EW_ACCUM;
    if (c < d.C) {
        const int nrows = d.B * d.Hi;
        for (int row = blockIdx.y; row < nrows; row += gridDim.y) {
            const int b = row / d.Hi, yi = row - b * d.Hi;
            const int kh0 = (yi + pad) & 1;
            for (int xi = ty; xi < d.Wi; xi += PY) {
                const int kw0 = (xi + pad) & 1;
                uint4 raw[KT][KT];
                bool ok[KT][KT];
#pragma unroll
                for (int a = 0; a < KT; ++a) {
                    const int kh = kh0 + 2 * a;
                    const int yo = (yi + pad - kh) >> 1;
                    const bool yok = kh < K && yo >= 0 && yo < d.Ho && yi + pad - kh >= 0;
#pragma unroll
                    for (int e = 0; e < KT; ++e) {
                        const int kw = kw0 + 2 * e;
                        const int xo = (xi + pad - kw) >> 1;
                        ok[a][e] = yok && kw < K && xo >= 0 && xo < d.Wo && xi + pad - kw >= 0;
                        raw[a][e] = *(const uint4*)(dy + (((long)b * d.Ho + dw_clamp(yo, d.Ho)) * d.Wo + dw_clamp(xo, d.Wo)) * d.ldy + c);
                    }
                }
                float acc[EPV];
#pragma unroll
                for (int j = 0; j < EPV; ++j) acc[j] = 0.f;
#pragma unroll
                for (int a = 0; a < KT; ++a)
#pragma unroll
                    for (int e = 0; e < KT; ++e) {
                        const int kh = kh0 + 2 * a, kw = kw0 + 2 * e;
                        const int t = (kh < K && kw < K) ? kh * K + kw : 0;
                        float xv[EPV], wv[EPV];
                        dw_load_f32<EPV>(d.w + (long)t * d.C + c, wv);
                        vec_unpack<T>(raw[a][e], xv);
                        const bool in = ok[a][e];
#pragma unroll
                        for (int j = 0; j < EPV; ++j) acc[j] += in ? xv[j] * wv[j] : 0.f;
                    }
                T* xp = dx + ((long)row * d.Wi + xi) * d.ldx + c;
                if (accum) {
                    float old[EPV];
                    vec_unpack<T>(*(const uint4*)xp, old);
#pragma unroll
                    for (int j = 0; j < EPV; ++j) acc[j] += old[j];
                }
                *(uint4*)xp = vec_pack<T>(acc);
            }
        }
    }
}

// dw[t][c] += sum_p dy[p][c] * x[src(p, t)][c].  grid.z = kernel row kh; a thread keeps the K taps of that row for its
// 8 channels in registers (K*8 accumulators), reads the output-gradient vector of a pixel once and the K input vectors of
// the row from L1 -- one pass over dy per kernel row instead of one per tap, K x fewer workgroup reductions and atomics.
template <typename T, int K>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(DykDwDesc d, int CVB) {
    constexpr int EPV = ElemTraits<T>::EPV;
    __shared__ float red[256 * 8];
    const int PY = 256 / CVB;
    const int tx = threadIdx.x % CVB, ty = threadIdx.x / CVB;
    const int cv = blockIdx.x * CVB + tx;
    const int c = cv * EPV;
    const bool active = c < d.C;
    const int kh = blockIdx.z;
    const T* __restrict__ x = (const T*)d.x;
    const T* __restrict__ dy = (const T*)d.y;       // output gradient [B,Ho,Wo,C]
    float acc[K][EPV];
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int j = 0; j < EPV; ++j) acc[t][j] = 0.f;
    // DykDwDesc.pre: x holds the raw output of the producing conv; z = dtype(act(scale * u + shift)) is formed on load
    const bool pre = d.pre != nullptr;
    float psc[EPV], psh[EPV];
#pragma unroll
    for (int j = 0; j < EPV; ++j) { psc[j] = 1.f; psh[j] = 0.f; }
    if (pre && active) {
#pragma unroll
        for (int j = 0; j < EPV; ++j) { psc[j] = d.pre[c + j]; psh[j] = d.pre[d.C + c + j]; }
    }
    const int pact = d.pre_act;
    const bool p_generic = pre && !(pact == DYK_ACT_LINEAR || pact == DYK_ACT_RELU || pact == DYK_ACT_RELU6 || pact == DYK_ACT_HSWISH ||
                                    pact == DYK_ACT_LEAKY);
    const float p_lo = (pact == DYK_ACT_RELU || pact == DYK_ACT_RELU6) ? 0.f : -__builtin_inff();
    const float p_hi = pact == DYK_ACT_RELU6 ? 6.f : __builtin_inff();
    const float p_leak = pact == DYK_ACT_LEAKY ? 0.1f : 1.f;
    const bool p_hsw = pact == DYK_ACT_HSWISH;
    auto pre_apply = [&](float (&xv)[EPV]) {
        if (pre) {
#pragma unroll
            for (int j = 0; j < EPV; ++j) {
                const float t = xv[j] * psc[j] + psh[j];
                float r = fminf(fmaxf(fmaxf(t, p_leak * t), p_lo), p_hi);
                if (p_hsw) r = t * fminf(fmaxf(t + 3.f, 0.f), 6.f) * (1.f / 6.f);
                if (p_generic) r = act_fwd(pact, t);
                xv[j] = r;
            }
            const uint4 pk = vec_pack<T>(xv);                  // rounded to the storage type: what the separate pass would have stored
            vec_unpack<T>(pk, xv);
        }
    };
    if (active) {
        const int nrows = d.B * d.Ho;
        for (int row = blockIdx.y; row < nrows; row += gridDim.y) {
          const int b = row / d.Ho, yo = row - b * d.Ho;
            const int yi = yo * d.stride + kh - d.pad;
            if (yi < 0 || yi >= d.Hi) continue;
            const T* xrow = x + ((long)b * d.Hi + yi) * d.Wi * d.ldx + c;
            if (d.stride == 1) {
                // strips of 4 output pixels: 4 gradient vectors + (4 + K - 1) input vectors per strip and kernel row
                constexpr int XT = 4;
                for (int xo0 = ty * XT; xo0 < d.Wo; xo0 += PY * XT) {
                    float g[XT][EPV];
                    // all loads of the strip first (clamped columns, values zeroed afterwards): one memory round trip
                    uint4 graw[XT], xraw[XT + K - 1];
#pragma unroll
                    for (int o = 0; o < XT; ++o) {
                        const int xo = xo0 + o < d.Wo ? xo0 + o : d.Wo - 1;
                        graw[o] = *(const uint4*)(dy + ((long)row * d.Wo + xo) * d.ldy + c);
                    }
#pragma unroll
                    for (int sl = 0; sl < XT + K - 1; ++sl)
                        xraw[sl] = *(const uint4*)(xrow + (long)dw_clamp(xo0 - d.pad + sl, d.Wi) * d.ldx);
#pragma unroll
                    for (int o = 0; o < XT; ++o) {
                        vec_unpack<T>(graw[o], g[o]);
                        const bool in = xo0 + o < d.Wo;
#pragma unroll
                        for (int j = 0; j < EPV; ++j) g[o][j] = in ? g[o][j] : 0.f;
                    }
#pragma unroll
                    for (int sl = 0; sl < XT + K - 1; ++sl) {
                        const int xi = xo0 - d.pad + sl;
                        const bool in = xi >= 0 && xi < d.Wi;
                        float xv[EPV];
                        vec_unpack<T>(xraw[sl], xv);
                        pre_apply(xv);
#pragma unroll
                        for (int j = 0; j < EPV; ++j) xv[j] = in ? xv[j] : 0.f;
#pragma unroll
                        for (int o = 0; o < XT; ++o) {
                            const int t = sl - o;                  // tap within the kernel row (compile-time after unrolling)
                            if (t < 0 || t >= K) continue;
#pragma unroll
                            for (int j = 0; j < EPV; ++j) acc[t][j] += g[o][j] * xv[j];
                        }
                    }
                }
                continue;
            }
          for (int xo = ty; xo < d.Wo; xo += PY) {
            const long p = (long)row * d.Wo + xo;
            float g[EPV];
            vec_unpack<T>(*(const uint4*)(dy + p * d.ldy + c), g);
            const int xi0 = xo * d.stride - d.pad;
            uint4 xraw[K];
#pragma unroll
            for (int t = 0; t < K; ++t) xraw[t] = *(const uint4*)(xrow + (long)dw_clamp(xi0 + t, d.Wi) * d.ldx);
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const int xi = xi0 + t;
                const bool in = xi >= 0 && xi < d.Wi;
                float xv[EPV];
                vec_unpack<T>(xraw[t], xv);
                pre_apply(xv);
#pragma unroll
                for (int j = 0; j < EPV; ++j) acc[t][j] += in ? g[j] * xv[j] : 0.f;
            }
          }
        }
    }
    // fold the pixel lanes through LDS, one tap at a time (8 floats per thread)
#pragma unroll
    for (int t = 0; t < K; ++t) {
        float* mine = red + threadIdx.x * 8;
#pragma unroll
        for (int j = 0; j < EPV; ++j) mine[j] = acc[t][j];
        __syncthreads();
        if (ty == 0 && active) {
            float s[EPV];
#pragma unroll
            for (int j = 0; j < EPV; ++j) s[j] = acc[t][j];
            for (int q = 1; q < PY; ++q) {
                const float* o = red + (q * CVB + tx) * 8;
#pragma unroll
                for (int j = 0; j < EPV; ++j) s[j] += o[j];
            }
            if (d.part) {          // plane mode: this workgroup row's own plane, plain stores
                float* pp = d.part + ((long)blockIdx.y * K * K + (kh * K + t)) * d.C + c;
#pragma unroll
                for (int j = 0; j < EPV; ++j) pp[j] = s[j];
            } else {
#pragma unroll
                for (int j = 0; j < EPV; ++j) unsafeAtomicAdd(d.dw + (long)(kh * K + t) * d.C + c + j, s[j]);
            }
        }
        __syncthreads();
    }
}

// LDS-tiled, PERSISTENT stride-1 depthwise weight gradient (bf16, k = 3 | 5; round 5).  dwconv_wgrad_kernel above makes K passes over dy
// and x (grid.z = kernel row) with 12 sixteen-byte loads in flight per thread and three waves per SIMD: ~0.6 MB in flight over the
// chip, 0.5-2 TB/s, waiting 0.64-0.74 of its cycles (tools/dw_pmc.sh).  Here a workgroup walks output tiles of TH x 16 pixels for
// CT <= 8 channel vectors (the geometry of dwconv_tile_kernel): the x patch and the dy tile of the NEXT tile are requested into
// registers (12 loads per thread, every one issued before anything waits) and stay in flight while the current tile is computed
// from LDS -- one pass over both tensors, halo re-reads only.  Thread = (channel vector, kernel row kh, pixel lane): K * 8
// accumulators, a strip of 4 pixels costs 4 + (4 + K - 1) ds_read_b128 for 4 * K * 8 multiply-adds.  Out-of-image patch pixels,
// pixels beyond the output extent and ragged tiles are zeros in LDS, so no tap needs a bounds test.  Workgroup wg of its channel
// group owns plane wg (DykDwDesc.part: plain stores, folded in plane order by dyk_grad_reduce -- same sums from run to run);
// without planes, one fp32 atomic per (tap, channel) and workgroup.
typedef __bf16 dw_bf16x2_t __attribute__((ext_vector_type(2)));
template <int K, bool PRE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void dwconv_wgrad_tile_kernel(DykDwDesc d, int CT, int groups, unsigned m_ct, int tiles_x,
                                                                int tiles_y, int P) {
    using T = bf16_t;
    constexpr int EPV = 8, TW = DW_TW, XT = DW_XT, SPR = DW_SPR, NS = XT + K - 1, IC = TW + K - 1;
    constexpr int NLX = dw_patch_loads(K), NLG = 4, NLD = NLX + NLG;     // loads per thread: x patch, dy tile (TH * TW * CT <= 4 * 256)
    extern __shared__ uint4 smem[];
    const int S = dw_slot_stride(CT);
    const int TH = dw_tile_rows(CT), IR = TH + K - 1;
    uint4* patch = smem;                                       // [IR][IC][S]  x
    uint4* gtile = smem + IR * IC * S;                         // [TH][TW][S]  dy
    const int tid = threadIdx.x;
    const int grp = blockIdx.x % groups, wg = blockIdx.x / groups;
    const int cv0 = grp * CT, CV = d.C / EPV;
    const T* __restrict__ x = (const T*)d.x;
    const T* __restrict__ dy = (const T*)d.y;
    const int ntiles = d.B * tiles_y * tiles_x;
    // ---- staging roles (the same for every tile): load i of this thread = vector (row, col, ct) of the patch / of the dy tile
    int role[NLD];                                             // row | col << 8 | ct << 16, -1 = none
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const bool isx = i < NLX;
        const unsigned idx = tid + (isx ? i : i - NLX) * 256;
        const unsigned q = CT == 1 ? idx : __umulhi(idx, m_ct);
        const int ct = (int)(idx - q * CT);
        const int w = isx ? IC : TW;
        const int row = (int)(q / w), col = (int)(q - (unsigned)row * w);
        const bool valid = idx < (unsigned)((isx ? IR * IC : TH * TW) * CT) && cv0 + ct < CV;
        role[i] = valid ? (row | (col << 8) | (ct << 16)) : -1;
    }
    uint4 v[NLD];
    unsigned okm = 0;
    auto request = [&](int t) __attribute__((always_inline)) {
        const int txi = t % tiles_x, r1 = t / tiles_x;
        const int tyi = r1 % tiles_y, b = r1 / tiles_y;
        const int y0 = tyi * TH, x0 = txi * TW;
        const T* ximg = x + (long)b * d.Hi * d.Wi * d.ldx + (long)cv0 * EPV;
        const T* gimg = dy + (long)b * d.Ho * d.Wo * d.ldy + (long)cv0 * EPV;
        okm = 0;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int ro = role[i] < 0 ? 0 : role[i];
            const int row = ro & 0xff, col = (ro >> 8) & 0xff, ct = ro >> 16;
            if (i < NLX) {
                const int ys = y0 + row - d.pad, xs = x0 + col - d.pad;
                const bool ok = role[i] >= 0 && ys >= 0 && ys < d.Hi && xs >= 0 && xs < d.Wi;
                v[i] = *(const uint4*)(ximg + ((long)dw_clamp(ys, d.Hi) * d.Wi + dw_clamp(xs, d.Wi)) * d.ldx + ct * EPV);
                okm |= ok ? (1u << i) : 0u;
            } else {
                const int ys = y0 + row, xs = x0 + col;
                const bool ok = role[i] >= 0 && ys < d.Ho && xs < d.Wo;
                const int yc = ys >= d.Ho ? d.Ho - 1 : ys, xc = xs >= d.Wo ? d.Wo - 1 : xs;
                v[i] = *(const uint4*)(gimg + ((long)yc * d.Wo + xc) * d.ldy + ct * EPV);
                okm |= ok ? (1u << i) : 0u;
            }
        }
    };
    // ---- compute role
    const int cct = tid % CT, rest = tid / CT;
    const int kh = rest % K, lane = rest / K;
    const int NL = (256 / CT) / K;
    const bool active = lane < NL && cv0 + cct < CV;
    float acc[K][EPV];
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int j = 0; j < EPV; ++j) acc[t][j] = 0.f;

    // DykDwDesc.pre (PRE): x holds the RAW output of the producing conv; z = dtype(act(scale * u + shift)) is formed between the
    // loads and the LDS stores -- the patch then holds exactly what the separate normalise pass would have stored.  Branch-free
    // for ReLU / ReLU6 / h-swish / leaky / linear: act(t) = clamp(max(t, leak * t), lo, hi), h-swish t * clamp(t + 3, 0, 6) / 6
    // (the same expressions as in dwconv_wgrad_kernel: DESIGN 5.4 relies on both giving the same bf16 values)
    float* pl = (float*)(smem + (IR * IC + TH * TW) * S);      // [2][CT * 8] scale | shift of this channel group
    const int pact = d.pre_act;
    const bool p_generic = !(pact == DYK_ACT_LINEAR || pact == DYK_ACT_RELU || pact == DYK_ACT_RELU6 || pact == DYK_ACT_HSWISH ||
                             pact == DYK_ACT_LEAKY);
    const float p_lo = (pact == DYK_ACT_RELU || pact == DYK_ACT_RELU6) ? 0.f : -__builtin_inff();
    const float p_hi = pact == DYK_ACT_RELU6 ? 6.f : __builtin_inff();
    const float p_leak = pact == DYK_ACT_LEAKY ? 0.1f : 1.f;
    const bool p_hsw = pact == DYK_ACT_HSWISH;
    if constexpr (PRE) {
        for (int i = tid; i < 2 * CT * 8; i += 256) {
            const int which = i / (CT * 8), rem = i - which * (CT * 8);
            const int cch = cv0 * EPV + rem;
            pl[i] = cch < d.C ? d.pre[(long)which * d.C + cch] : 0.f;
        }
    }

    int t = wg;
    if (t < ntiles) request(t);
    for (; t < ntiles; t += P) {
        __syncthreads();                                       // the previous tile's LDS reads are done (and, first trip, pl is there)
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            if (role[i] < 0) continue;
            const int row = role[i] & 0xff, col = (role[i] >> 8) & 0xff, ct = role[i] >> 16;
            if constexpr (PRE) {
                if (i < NLX) {
                    float u[EPV];
                    vec_unpack<T>(v[i], u);
#pragma unroll
                    for (int j = 0; j < EPV; ++j) {
                        const float tt = u[j] * pl[ct * 8 + j] + pl[CT * 8 + ct * 8 + j];
                        float r = fminf(fmaxf(fmaxf(tt, p_leak * tt), p_lo), p_hi);
                        if (p_hsw) r = tt * fminf(fmaxf(tt + 3.f, 0.f), 6.f) * (1.f / 6.f);
                        if (p_generic) r = act_fwd(pact, tt);
                        u[j] = r;
                    }
                    v[i] = vec_pack<T>(u);
                }
            }
            const uint4 z = ((okm >> i) & 1u) ? v[i] : make_uint4(0u, 0u, 0u, 0u);
            if (i < NLX) patch[(row * IC + col) * S + ct] = z;
            else gtile[(row * TW + col) * S + ct] = z;
        }
        __syncthreads();
        if (t + P < ntiles) request(t + P);                    // in flight while this tile is computed
        if (active) {
#pragma unroll 1
            for (int s = lane; s < TH * SPR; s += NL) {
                const int r = s / SPR, strip = s - r * SPR;
                const uint4* grow = gtile + (r * TW + strip * XT) * S + cct;
                const uint4* prow = patch + ((r + kh) * IC + strip * XT) * S + cct;
                // v_dot2c_f32_bf16: acc += x.lo * g.lo + x.hi * g.hi on the PACKED pairs -- with one half of g masked to zero
                // it is the fp32 multiply-add of one channel (a bf16 x bf16 product is exact in fp32: one rounding, as the
                // fma), and the x vectors need no unpacking: 8 VALU ops fewer per input vector.
                // PROPERTY: the unmasked neighbour half of x still meets the zero half of g, so a NON-FINITE x in
                // channel c ^ 1 turns the gradient of channel c into NaN (0 * Inf) where the row kernel (fp32 fma per channel,
                // stride 2 / fp32 shapes) keeps the channels apart; finite inputs give the same sums as that kernel up to the
                // summation order.  Masking x as well would put the 8 VALU ops per vector back that this form saves; a
                // non-finite activation already poisons the step's loss (GradScaler skips it), so the forms are not unified.
                unsigned gm[XT][EPV];
#pragma unroll
                for (int o = 0; o < XT; ++o) {
                    const uint4 gr = grow[o * S];
                    const unsigned gw[4] = {gr.x, gr.y, gr.z, gr.w};
#pragma unroll
                    for (int m = 0; m < 4; ++m) { gm[o][2 * m] = gw[m] & 0xffffu; gm[o][2 * m + 1] = gw[m] & 0xffff0000u; }
                }
#pragma unroll
                for (int q = 0; q < NS; ++q) {
                    const uint4 xr = prow[q * S];
                    const unsigned xw[4] = {xr.x, xr.y, xr.z, xr.w};
#pragma unroll
                    for (int o = 0; o < XT; ++o) {
                        const int tp = q - o;
                        if (tp < 0 || tp >= K) continue;
#pragma unroll
                        for (int j = 0; j < EPV; ++j)
                            acc[tp][j] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dw_bf16x2_t, xw[j >> 1]),
                                                                         __builtin_bit_cast(dw_bf16x2_t, gm[o][j]), acc[tp][j], false);
                    }
                }
            }
        }
    }
    // ---- fold the pixel lanes through LDS in lane order, one tap at a time; plane = this workgroup of its channel group.
    // (the fold of dwconv_wgrad_kernel with lane stride K * CT and a float4 store; written out in both, see the note on helpers
    // at the top of the file)
    __syncthreads();
    float* red = (float*)smem;
#pragma unroll
    for (int tp = 0; tp < K; ++tp) {
        float* mine = red + tid * 8;
#pragma unroll
        for (int j = 0; j < EPV; ++j) mine[j] = acc[tp][j];
        __syncthreads();
        if (active && lane == 0) {
            float sum[EPV];
#pragma unroll
            for (int j = 0; j < EPV; ++j) sum[j] = acc[tp][j];
            for (int q = 1; q < NL; ++q) {
                const float* o = red + ((q * K + kh) * CT + cct) * 8;
#pragma unroll
                for (int j = 0; j < EPV; ++j) sum[j] += o[j];
            }
            const int c = (cv0 + cct) * EPV;
            if (d.part) {
                float* pp = d.part + ((long)wg * K * K + (kh * K + tp)) * d.C + c;
                if (((size_t)pp & 15) == 0) {
                    *(float4*)pp = make_float4(sum[0], sum[1], sum[2], sum[3]);
                    *(float4*)(pp + 4) = make_float4(sum[4], sum[5], sum[6], sum[7]);
                } else {
#pragma unroll
                    for (int j = 0; j < EPV; ++j) pp[j] = sum[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < EPV; ++j) unsafeAtomicAdd(d.dw + (long)(kh * K + tp) * d.C + c + j, sum[j]);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- host: geometry and routes
// geometry of the LDS-tiled kernels for C channels, kernel size k (3 | 5) and B output maps of Hout x Wout.  CT is 1..8 by
// construction, and the patch of every CT fits the staging loads (nvec of nld):
//   CT          1     2     3     4     5     6     7     8
//   k = 3    1188  1224  1242  1296  1260  1296  1386  1440   of 1536
//   k = 5    1360  1440  1500  1600  1600  1680  1820  1920   of 2048
struct DwGeom {
    int CT, groups, S, TH, IR, IC, tiles_x, tiles_y;
    int nvec, nld;              // patch vectors, and the staging limit they must fit: dw_patch_loads(k) * 256
    unsigned m_ct;              // idx / CT == umulhi(idx, m_ct) for idx < 2^32 / CT
    long ntiles;                // B * tiles_y * tiles_x
    bool fits() const { return nvec <= nld; }
};
inline DwGeom dw_tile_geometry(int C, int k, int Hout, int Wout, int B) {
    DwGeom g;
    const int CV = C / 8;
    g.groups = (CV + 7) / 8;
    g.CT = (CV + g.groups - 1) / g.groups;
    g.S = dw_slot_stride(g.CT);
    g.TH = dw_tile_rows(g.CT);
    g.IR = g.TH + k - 1;
    g.IC = DW_TW + k - 1;
    g.tiles_x = (Wout + DW_TW - 1) / DW_TW;
    g.tiles_y = (Hout + g.TH - 1) / g.TH;
    g.nvec = g.IR * g.IC * g.CT;
    g.nld = dw_patch_loads(k) * 256;
    g.m_ct = (unsigned)(0xFFFFFFFFu / (unsigned)g.CT) + 1u;
    g.ntiles = (long)B * g.tiles_x * g.tiles_y;
    return g;
}

// What an entry point does with a checked descriptor: a return code, or the kernel with its launch parameters.  The kernels take
// (d, CVB) on a dw_route_rows grid, or, tiled, (d, CT, groups, m_ct, tiles_x, tiles_y [, P]) on the tile geometry
struct DwRoute {
    int rc;
    const void* kernel;         // null: no instantiation for this k (dw_route_wgrad)
    bool tiled;
    dim3 grid;
    size_t lds;
    DwGeom g;                   // tiled
    int CVB;                    // rows
    int planes;                 // weight gradient: workgroup rows (rows) | workgroups per channel group P (tiled)
};
inline DwRoute dw_refuse(int rc) { DwRoute r = {}; r.rc = rc; return r; }
// the K in {3, 5} instantiation of a kernel template whose first parameter is K
#define DW_K35(k, KERNEL, ...) ((k) == 3 ? (const void*)KERNEL<3, __VA_ARGS__> : (const void*)KERNEL<5, __VA_ARGS__>)

int check_dw(const DykDwDesc* d) {
    if (!d || !d->x || !d->y || d->B <= 0 || d->C <= 0 || d->k <= 0 || d->k > 7 || d->stride <= 0) return DYK_ERR_ARG;
    if (d->dtype != DYK_BF16 && d->dtype != DYK_F32 && d->dtype != DYK_F16) return DYK_ERR_ARG;
    const int epv = d->dtype == DYK_F32 ? 4 : 8;
    if (d->C % epv || d->ldx % epv || d->ldy % epv) return DYK_ERR_ARG;
    if (d->Hi <= 0 || d->Wi <= 0 || d->Ho <= 0 || d->Wo <= 0) return DYK_ERR_ARG;
    return DYK_OK;
}

// a (d, CVB) kernel: grid.x = channel-vector groups, grid.y = image rows (strided), capped at cap_blocks workgroups
inline DwRoute dw_route_rows(const DykDwDesc* d, const void* fn, long nrows, int cap_blocks, int gz = 1) {
    DwRoute r = {};
    r.kernel = fn;
    const int CV = d->C / (d->dtype == DYK_F32 ? 4 : 8);
    r.CVB = 1;
    while (r.CVB < CV && r.CVB < 32) r.CVB <<= 1;
    const int gx = (CV + r.CVB - 1) / r.CVB;
    long g = nrows;
    const long cap = cap_blocks / gx > 0 ? cap_blocks / gx : 1;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    r.grid = dim3(gx, (unsigned)g, gz);
    r.planes = (int)g;
    return r;
}

// the shapes of the LDS-tiled kernels; the forward takes them in both 16-bit types (dyk_dwconv_tile_ok), the gradients in bf16
inline bool dw_k35_s1(const DykDwDesc* d) { return d->stride == 1 && (d->k == 3 || d->k == 5); }
inline bool dw_fwd_tiled_domain(const DykDwDesc* d) { return dw_k35_s1(d) && (d->dtype == DYK_BF16 || d->dtype == DYK_F16); }

// the LDS-tiled forward / data gradient.  Every problem of its domain runs: the patch always fits (table above) and LDS stays
// below 64 KB (k = 3: 29.4 KB at most, k = 5: 40.5 KB); what is left to refuse is a grid of 2^31 workgroups
inline DwRoute dw_route_tiled(const DykDwDesc* d, bool grad) {
    DwRoute r = {};
    const DwGeom& g = r.g = dw_tile_geometry(d->C, d->k, grad ? d->Hi : d->Ho, grad ? d->Wi : d->Wo, d->B);
    if (!g.fits()) return dw_refuse(DYK_ERR_UNSUPPORTED);
    r.lds = (size_t)g.IR * g.IC * g.S * 16 + (size_t)d->k * d->k * g.CT * 8 * 4 + (size_t)g.CT * 16 * 4;   // patch | weights | pre scale, shift
    if (r.lds < 256 * 16 * 4 + 2048) r.lds = 256 * 16 * 4 + 2048;            // the statistics reduction reuses the patch
    if (g.groups * g.ntiles >= (1L << 31) || r.lds > 64 * 1024) return dw_refuse(DYK_ERR_UNSUPPORTED);
    r.tiled = true;
    r.kernel = grad                 ? DW_K35(d->k, dwconv_tile_kernel, true, bf16_t)
             : d->dtype == DYK_F16 ? DW_K35(d->k, dwconv_tile_kernel, false, f16_t)
                                   : DW_K35(d->k, dwconv_tile_kernel, false, bf16_t);
    r.grid = dim3((unsigned)(g.groups * g.ntiles));
    return r;
}

DwRoute dw_route_fwd(const DykDwDesc* d) {
    if (!d->w) return dw_refuse(DYK_ERR_ARG);
    // fp16 is the inference type: the same kernel choice as bf16, no BatchNorm statistics, no normalise-on-load (train-mode forms)
    if (d->dtype == DYK_F16 && (d->stats || d->pre)) return dw_refuse(DYK_ERR_UNSUPPORTED);
    if (dw_fwd_tiled_domain(d)) return dw_route_tiled(d, false);
    if (d->pre) return dw_refuse(DYK_ERR_UNSUPPORTED);       // normalise + activation on load: the LDS-tiled kernel only
    // (stride 2 too: the generic kernel measured faster than a forward with compile-time taps)
    return dw_route_rows(d, d->dtype == DYK_BF16  ? (const void*)dwconv_kernel<bf16_t, false>
                            : d->dtype == DYK_F16 ? (const void*)dwconv_kernel<f16_t, false>
                                                  : (const void*)dwconv_kernel<float, false>,
                         (long)d->B * d->Ho, 4096);
}

DwRoute dw_route_dgrad(const DykDwDesc* d) {
    if (d->dtype == DYK_F16) return dw_refuse(DYK_ERR_UNSUPPORTED);
    if (!d->w) return dw_refuse(DYK_ERR_ARG);
    const bool k35 = (d->k == 3 || d->k == 5) && d->dtype == DYK_BF16;
    if (d->res) {                    // fused BatchNorm-backward reduce: LDS-tiled kernel only, no accumulate form
        if (!d->bn || !d->stats || d->stats_slots <= 0 || d->ldr < d->C || d->ldr % 8 || ((uintptr_t)d->res % 16)) return dw_refuse(DYK_ERR_ARG);
        if (!(k35 && d->stride == 1) || (d->flags & DYK_EW_ACCUM)) return dw_refuse(DYK_ERR_UNSUPPORTED);
    }
    if (k35 && d->stride == 1) return dw_route_tiled(d, true);
    return dw_route_rows(d, k35 && d->stride == 2   ? DW_K35(d->k, dwconv_s2_dgrad_kernel, bf16_t)
                            : d->dtype == DYK_BF16 ? (const void*)dwconv_kernel<bf16_t, true>
                                                   : (const void*)dwconv_kernel<float, true>,
                         (long)d->B * d->Hi, 4096);
}

template <typename T>
const void* dw_wgrad_rows_kernel(int k) {
    switch (k) {
    case 1: return (const void*)dwconv_wgrad_kernel<T, 1>;
    case 3: return (const void*)dwconv_wgrad_kernel<T, 3>;
    case 5: return (const void*)dwconv_wgrad_kernel<T, 5>;
    case 7: return (const void*)dwconv_wgrad_kernel<T, 7>;
    default: return nullptr;
    }
}

// The persistent tiled kernel where it is eligible (bf16, stride 1, k = 3 | 5), else the row kernel.  The weight gradient adds to
// the shared geometry only what is its own: the dy tile and its LDS layout, IR <= 255 (the staging roles pack a row into 8 bits),
// at least one pixel lane per kernel row, ntiles < 2^30, and P.  An even k gets the row kernel's grid and plane count but no
// kernel: dyk_dwconv_wgrad_rows answers the planes, dyk_dwconv_wgrad refuses the launch (as recorded in dwconv_queries.json)
DwRoute dw_route_wgrad(const DykDwDesc* d) {
    if (d->dtype == DYK_F16) return dw_refuse(DYK_ERR_UNSUPPORTED);
    if (d->dtype == DYK_BF16 && dw_k35_s1(d)) {
        DwRoute r = {};
        const DwGeom& g = r.g = dw_tile_geometry(d->C, d->k, d->Ho, d->Wo, d->B);
        r.lds = (size_t)(g.IR * g.IC + g.TH * DW_TW) * g.S * 16 + (size_t)2 * g.CT * 8 * 4;      // patch | dy tile | pre scale, shift
        if (r.lds < 256 * 8 * 4) r.lds = 256 * 8 * 4;                                            // the lane fold reuses the patch
        if (g.fits() && (256 / g.CT) / d->k >= 1 && g.IR <= 255 && g.ntiles < (1L << 30) && r.lds <= 64 * 1024) {
            // 512 workgroups per launch, two resident per CU (three for the 3x3 kernel at 164 VGPRs measured equal: 70 / 87 /
            // 20 / 29 us against 65 / 88 / 20 / 29), the tiles dealt evenly over the rounds
            long p0 = 512 / g.groups;
            if (p0 < 1) p0 = 1;
            if (p0 > g.ntiles) p0 = g.ntiles;
            const long rounds = (g.ntiles + p0 - 1) / p0;
            r.planes = (int)((g.ntiles + rounds - 1) / rounds);
            r.tiled = true;
            r.kernel = d->pre ? DW_K35(d->k, dwconv_wgrad_tile_kernel, true) : DW_K35(d->k, dwconv_wgrad_tile_kernel, false);
            r.grid = dim3((unsigned)(g.groups * r.planes));
            return r;
        }
    }
    // few, long-running workgroups: every workgroup ends with one atomic per (tap, channel) on only k*k*C addresses
    return dw_route_rows(d, d->dtype == DYK_BF16 ? dw_wgrad_rows_kernel<bf16_t>(d->k) : dw_wgrad_rows_kernel<float>(d->k), (long)d->B * d->Ho,
                         768 / d->k, d->k);
}

int dw_launch(const DykDwDesc* d, const DwRoute& r, hipStream_t s) {
    if (r.rc != DYK_OK) return r.rc;
    if (!r.kernel) return DYK_ERR_UNSUPPORTED;
    DykDwDesc desc = *d;
    DwGeom g = r.g;
    int CVB = r.CVB, P = r.planes;
    void* rows_args[] = {&desc, &CVB};
    void* tile_args[] = {&desc, &g.CT, &g.groups, &g.m_ct, &g.tiles_x, &g.tiles_y, &P};    // P: the weight gradient only
    if (hipLaunchKernel(r.kernel, r.grid, dim3(256), r.tiled ? tile_args : rows_args, r.lds, s) != hipSuccess) return DYK_ERR_HIP;
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

}  // namespace

extern "C" int dyk_dwconv_fwd(const DykDwDesc* d, void* stream) {
    const int rc = check_dw(d);
    return rc ? rc : dw_launch(d, dw_route_fwd(d), (hipStream_t)stream);
}

extern "C" int dyk_dwconv_tile_ok(const DykDwDesc* d) {
    const int rc = check_dw(d);
    return rc ? rc : (dw_fwd_tiled_domain(d) && dw_route_tiled(d, false).rc == DYK_OK ? 1 : 0);
}

extern "C" int dyk_dwconv_dgrad(const DykDwDesc* d, void* stream) {
    const int rc = check_dw(d);
    return rc ? rc : dw_launch(d, dw_route_dgrad(d), (hipStream_t)stream);
}

extern "C" int dyk_dwconv_wgrad_rows(const DykDwDesc* d) {
    const int rc = check_dw(d);
    if (rc) return rc;
    const DwRoute r = dw_route_wgrad(d);
    return r.rc != DYK_OK ? r.rc : r.planes;
}

extern "C" int dyk_dwconv_wgrad(const DykDwDesc* d, void* stream) {
    const int rc = check_dw(d);
    if (rc) return rc;
    const DwRoute r = dw_route_wgrad(d);
    if (r.rc == DYK_OK && !d->dw) return DYK_ERR_ARG;
    return dw_launch(d, r, (hipStream_t)stream);
}
