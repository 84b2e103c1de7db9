// Non-finite guard and gradient clipping for the fused optimizers, decided on the device (what the reference harness gets from
// amp.GradScaler, train_utils/kaist_train_eval_utils.py:44,103-108, and from torch.nn.utils.clip_grad_norm_): one fp64 reduction
// over the flat gradient buffer in two launches (block partials, then one workgroup that folds them in block order and writes a
// small record).  The step kernel of optim.hip takes skip / clip coefficient / bias corrections from that record instead of
// from the host; dyk_grad_scale_by_rec applies the coefficient to the gradient for users of stock torch.optim.  No atomics and no
// in-launch hand-off: the kernel boundary orders the partials before the fold, and the fold before the step.  HBM-bound: 16-byte
// vectors, four loads in flight per lane; per loaded float one fp32 product, one conversion and one fp64 FMA (a few per cent of
// the fp64 vector rate at HBM speed).
#include <float.h>
#include "dyk_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;      // 4 workgroups per CU; the fold reads at most 1024 partials
constexpr int kUnroll = 4;

struct alignas(16) GradPartial {
    double sumsq;
    uint32_t nonfinite;
    uint32_t _pad;
};

inline long stats_blocks(long n) {
    long g = ((n >> 2) + kBlock - 1) / kBlock;
    return g > kMaxBlocks ? kMaxBlocks : g;
}

__device__ __forceinline__ void take(const float4& v, float gs, double& acc, uint32_t& bad) {
    const float* e = (const float*)&v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x = __fmul_rn(e[j], gs);
        bad += !(fabsf(x) <= FLT_MAX) ? 1u : 0u;
        const double xd = (double)x;
        acc = __fma_rn(xd, xd, acc);                              // xd*xd is exact (48 bits): one rounding, FMA or not
    }
}

template <bool MASKED>
__global__ __launch_bounds__(kBlock) void stats_partials_kernel(const float4* __restrict__ g, const uint32_t* __restrict__ mask,
                                                                long n4, float gs, GradPartial* __restrict__ ws) {
    const long stride = (long)gridDim.x * kBlock;
    long i = blockIdx.x * (long)kBlock + threadIdx.x;
    double acc = 0.0;
    uint32_t bad = 0;
    for (; i + (kUnroll - 1) * stride < n4; i += kUnroll * stride) {
        uint32_t live[kUnroll];
        float4 v[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) live[k] = MASKED ? mask[i + k * stride] : 1u;
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) v[k] = live[k] ? g[i + k * stride] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
            if (live[k]) take(v[k], gs, acc, bad);
    }
    for (; i < n4; i += stride) {
        if (MASKED && mask[i] == 0) continue;                     // frozen parameters (entries are 64-element aligned)
        take(g[i], gs, acc, bad);
    }
    // fixed tree: lanes (l += l+32, l+16, ..., l+1), then the four waves in order
#pragma unroll
    for (int off = DYK_WAVE / 2; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off);
        bad += __shfl_down(bad, off);
    }
    __shared__ double s_acc[kBlock / DYK_WAVE];
    __shared__ uint32_t s_bad[kBlock / DYK_WAVE];
    if ((threadIdx.x & (DYK_WAVE - 1)) == 0) {
        s_acc[threadIdx.x / DYK_WAVE] = acc;
        s_bad[threadIdx.x / DYK_WAVE] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = s_acc[0];
        uint32_t b = s_bad[0];
#pragma unroll
        for (int w = 1; w < kBlock / DYK_WAVE; ++w) {
            a += s_acc[w];
            b += s_bad[w];
        }
        GradPartial out;
        out.sumsq = a;
        out.nonfinite = b;
        out._pad = 0;
        ws[blockIdx.x] = out;
    }
}

// beta^t for an integer t >= 0, rounded once to double: square-and-multiply on double-double values (error ~2^-100 before the
// final rounding), i.e. the correctly rounded power that the host's pow() returns in dyk_adam_step
struct dd {
    double hi, lo;
};
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
    const double p = __dmul_rn(a.hi, b.hi);
    double e = __fma_rn(a.hi, b.hi, -p);
    e = __fma_rn(a.hi, b.lo, e);
    e = __fma_rn(a.lo, b.hi, e);
    const double s = __dadd_rn(p, e);
    dd r;
    r.hi = s;
    r.lo = __dadd_rn(e, -__dadd_rn(s, -p));
    return r;
}
__device__ double pow_int(double b, int t) {
    dd r = {1.0, 0.0}, x = {b, 0.0};
    while (t > 0) {
        if (t & 1) r = dd_mul(r, x);
        t >>= 1;
        if (t) x = dd_mul(x, x);
    }
    return __dadd_rn(r.hi, r.lo);
}

__global__ __launch_bounds__(kBlock) void stats_finalize_kernel(const GradPartial* __restrict__ ws, int nb, DykGradGuardRec* rec,
                                                                float max_norm, float beta1, float beta2, int skip_nonfinite) {
    __shared__ double s_sum[kMaxBlocks];
    __shared__ uint32_t s_cnt[kMaxBlocks];
    for (int i = threadIdx.x; i < nb; i += kBlock) {
        const GradPartial p = ws[i];
        s_sum[i] = p.sumsq;
        s_cnt[i] = p.nonfinite;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sumsq = 0.0;
    unsigned long long cnt = 0;
#pragma unroll 8
    for (int i = 0; i < nb; ++i) {                                // block-index order
        sumsq += s_sum[i];
        cnt += s_cnt[i];
    }
    const float norm = (float)sqrt(sumsq);
    const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
    const float coef = max_norm > 0.f ? (c > 1.f ? 1.f : c) : 1.f;
    const uint32_t nonfinite = cnt > 0xffffffffull ? 0xffffffffu : (uint32_t)cnt;
    const int skip = (skip_nonfinite && nonfinite > 0) ? 1 : 0;
    rec->sumsq = sumsq;
    rec->norm = norm;
    rec->coef = coef;
    rec->nonfinite = nonfinite;
    rec->skip = skip;
    if (!skip) {
        const int t = rec->applied + 1;
        rec->applied = t;
        rec->bc1 = (float)(1.0 - pow_int((double)beta1, t));
        rec->bc2_sqrt = (float)sqrt(1.0 - pow_int((double)beta2, t));
    } else {
        rec->skipped = rec->skipped + 1;
    }
}

__global__ __launch_bounds__(256) void scale_by_rec_kernel(float4* __restrict__ g, const uint32_t* __restrict__ mask, long n4,
                                                           const DykGradGuardRec* __restrict__ rec) {
    const float coef = rec->coef;
    if (coef == 1.0f) return;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        if (mask && mask[i] == 0) continue;
        float4 v = g[i];
        v.x = __fmul_rn(v.x, coef);
        v.y = __fmul_rn(v.y, coef);
        v.z = __fmul_rn(v.z, coef);
        v.w = __fmul_rn(v.w, coef);
        g[i] = v;
    }
}

}  // namespace

extern "C" int64_t dyk_grad_stats_ws_bytes(int64_t n) {
    if (n <= 0 || (n & 3)) return 0;
    return (int64_t)sizeof(GradPartial) * stats_blocks(n);
}

extern "C" int dyk_grad_stats(const DykGradStatsDesc* d, void* stream) {
    if (!d || !d->g || !d->ws || !d->rec || d->n <= 0 || (d->n & 3)) return DYK_ERR_ARG;
    if (((uintptr_t)d->g | (uintptr_t)d->ws) & 15) return DYK_ERR_ARG;
    if ((uintptr_t)d->rec & 7) return DYK_ERR_ARG;
    if (d->mask && ((uintptr_t)d->mask & 3)) return DYK_ERR_ARG;
    if (d->ws_bytes < dyk_grad_stats_ws_bytes(d->n)) return DYK_ERR_ARG;
    const long nb = stats_blocks(d->n);
    const float4* g = (const float4*)d->g;
    GradPartial* ws = (GradPartial*)d->ws;
    if (d->mask)
        hipLaunchKernelGGL(stats_partials_kernel<true>, dim3((int)nb), dim3(kBlock), 0, (hipStream_t)stream, g,
                           (const uint32_t*)d->mask, (long)(d->n >> 2), d->grad_scale, ws);
    else
        hipLaunchKernelGGL(stats_partials_kernel<false>, dim3((int)nb), dim3(kBlock), 0, (hipStream_t)stream, g,
                           (const uint32_t*)nullptr, (long)(d->n >> 2), d->grad_scale, ws);
    DYK_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const GradPartial*)ws, (int)nb,
                       d->rec, d->max_norm, d->beta1, d->beta2, d->skip_nonfinite);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_grad_scale_by_rec(float* g, const uint8_t* mask, int64_t n, const DykGradGuardRec* rec, void* stream) {
    if (!g || !rec || n <= 0 || (n & 3)) return DYK_ERR_ARG;
    if (((uintptr_t)g & 15) || ((uintptr_t)rec & 7) || (mask && ((uintptr_t)mask & 3))) return DYK_ERR_ARG;
    const long blocks = ((n >> 2) + 255) / 256;
    hipLaunchKernelGGL(scale_by_rec_kernel, dim3((int)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, (hipStream_t)stream, (float4*)g,
                       (const uint32_t*)mask, (long)(n >> 2), rec);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
