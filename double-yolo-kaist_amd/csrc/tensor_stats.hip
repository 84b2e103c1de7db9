// Per-tensor statistics over the flat parameter store (dyk_tensor_stats, include/dyk_hip.h): sum of squares, largest magnitude,
// non-finite and zero counts per (segment, buffer) for up to four flat fp32 buffers that share one segment table -- what a host
// loop of p.grad.norm() / torch.isfinite(p.grad) over some 600 views gives, in two launches and without a synchronisation.
// The style of optim_guard.hip: no atomics and no in-launch hand-off, the kernel boundary orders the item partials before the
// fold.  HBM-bound: 16-byte vectors, four loads per buffer in flight per lane; per loaded float two fp32 compares, one
// conversion and one fp64 FMA.  The ORDER of every addition is part of the interface (header): tests/tensor_stats_ref.py
// restates it and the tests hold sumsq to it bit for bit.
#include <float.h>
#include "dyk_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / DYK_WAVE;
constexpr int kItem = DYK_TSTAT_ITEM;                // elements per work item
constexpr int kVecs = kItem / 4 / kBlock;            // 16-byte vectors per thread and buffer: 4
static_assert(kVecs * kBlock * 4 == kItem, "an item is a whole number of vectors per thread");
static_assert(sizeof(DykTensorStat) == 24 && sizeof(DykTensorSeg) == 24 && sizeof(DykTensorItem) == 16, "ABI layout");

struct Acc {
    double sumsq;
    float amax;
    uint32_t cnt;          // nonfinite | zeros << 16: an item holds 4096 elements, either count fits 16 bits
};

// one vector; `live` = how many of its leading elements belong to the item (>= 4: all of them)
template <bool MASKED>
__device__ __forceinline__ void take(const float4& v, int live, Acc& a) {
    const float* e = (const float*)&v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = !MASKED || j < live;
        const float ax = fabsf(e[j]);
        const bool fin = ax <= FLT_MAX;
        a.cnt += (in && !fin ? 1u : 0u) + (in && ax == 0.f ? 0x10000u : 0u);
        const float x = (in && fin) ? ax : 0.f;      // left out: an exact zero, which changes no bit of the sums below
        const double xd = (double)x;
        a.sumsq = __fma_rn(xd, xd, a.sumsq);         // xd*xd is exact (48 bits): one rounding
        a.amax = fmaxf(a.amax, x);
    }
}

template <int NBUF>
struct Bufs {
    const float* p[NBUF];
};

template <int NBUF>
__global__ __launch_bounds__(kBlock) void tstat_partials_kernel(Bufs<NBUF> bufs, const DykTensorSeg* __restrict__ segs,
                                                                const DykTensorItem* __restrict__ items, int nseg, long n,
                                                                DykTensorStat* __restrict__ ws) {
    const int item = blockIdx.x;
    const DykTensorItem it = items[item];
    // the tables live in device memory: an entry that does not describe elements of its own segment inside [0, n) reads nothing
    bool ok = it.seg >= 0 && it.seg < nseg && it.len >= 1 && it.len <= kItem && it.first >= 0 && !(it.first & 3);
    uint32_t flags = 0;
    if (ok) {
        const DykTensorSeg sg = segs[it.seg];
        flags = sg.flags;
        ok = sg.offset >= 0 && sg.numel >= 1 && sg.offset <= n && sg.numel <= n - sg.offset && it.first >= sg.offset &&
             it.first - sg.offset <= sg.numel - it.len;
    }
    const int len = ok ? it.len : 0;
    const int t = threadIdx.x;
    __shared__ double s_sum[NBUF][kWaves];
    __shared__ float s_max[NBUF][kWaves];
    __shared__ uint32_t s_cnt[NBUF][kWaves];
    Acc acc[NBUF];
    float4 v[NBUF][kVecs];
#pragma unroll
    for (int k = 0; k < NBUF; ++k) {
        acc[k].sumsq = 0.0;
        acc[k].amax = 0.f;
        acc[k].cnt = 0;
        const bool skip = (flags >> k) & 1u;
        const float4* src = (const float4*)(bufs.p[k] + it.first);
#pragma unroll
        for (int u = 0; u < kVecs; ++u) {
            const int vi = t + u * kBlock;           // vector of the item; its elements are 4 vi .. 4 vi + 3
            v[k][u] = (!skip && 4 * vi < len) ? src[vi] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
#pragma unroll
    for (int k = 0; k < NBUF; ++k) {
        const bool skip = (flags >> k) & 1u;
        if (!skip) {
            if (len == kItem) {                      // a whole item: nothing to mask (uniform over the workgroup)
#pragma unroll
                for (int u = 0; u < kVecs; ++u) take<false>(v[k][u], 4, acc[k]);
            } else {
#pragma unroll
                for (int u = 0; u < kVecs; ++u) {
                    const int live = len - 4 * (t + u * kBlock);
                    if (live > 0) take<true>(v[k][u], live, acc[k]);
                }
            }
        }
        // fixed tree: lanes (l += l+32, l+16, ..., l+1), then the four waves in order
#pragma unroll
        for (int off = DYK_WAVE / 2; off > 0; off >>= 1) {
            acc[k].sumsq += __shfl_down(acc[k].sumsq, off);
            acc[k].amax = fmaxf(acc[k].amax, __shfl_down(acc[k].amax, off));
            acc[k].cnt += __shfl_down(acc[k].cnt, off);
        }
        if ((t & (DYK_WAVE - 1)) == 0) {
            s_sum[k][t / DYK_WAVE] = acc[k].sumsq;
            s_max[k][t / DYK_WAVE] = acc[k].amax;
            s_cnt[k][t / DYK_WAVE] = acc[k].cnt;
        }
    }
    __syncthreads();
    if (t < NBUF) {
        double a = s_sum[t][0];
        float m = s_max[t][0];
        uint32_t bad = s_cnt[t][0] & 0xffffu, zer = s_cnt[t][0] >> 16;
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            a += s_sum[t][w];
            m = fmaxf(m, s_max[t][w]);
            bad += s_cnt[t][w] & 0xffffu;
            zer += s_cnt[t][w] >> 16;
        }
        DykTensorStat out;
        out.sumsq = a;
        out.absmax = m;
        out.nonfinite = bad;
        out.zeros = zer;
        out._pad = 0;
        ws[(long)item * NBUF + t] = out;
    }
}

__global__ __launch_bounds__(kBlock) void tstat_fold_kernel(const DykTensorStat* __restrict__ ws, const DykTensorSeg* __restrict__ segs,
                                                            int nseg, int nitems, int nbuf, DykTensorStat* __restrict__ out) {
    const int s = blockIdx.x * kWaves + threadIdx.x / DYK_WAVE;      // one wave per segment
    if (s >= nseg) return;
    const int lane = threadIdx.x & (DYK_WAVE - 1);
    const DykTensorSeg sg = segs[s];
    const long cnt = sg.numel >= 1 ? (sg.numel + kItem - 1) / kItem : 0;
    const bool ok = cnt >= 1 && sg.item_begin >= 0 && cnt <= (long)nitems - sg.item_begin;
    const int b = sg.item_begin, c = ok ? (int)cnt : 0;
    for (int k = 0; k < nbuf; ++k) {
        double a = 0.0;
        float m = 0.f;
        unsigned long long bad = 0, zer = 0;
        if (!((sg.flags >> k) & 1u)) {
            for (int i = lane; i < c; i += DYK_WAVE) {               // lane l: partials b + l, b + l + 64, ... in that order
                const DykTensorStat p = ws[(long)(b + i) * nbuf + k];
                a += p.sumsq;
                m = fmaxf(m, p.absmax);
                bad += p.nonfinite;
                zer += p.zeros;
            }
        }
#pragma unroll
        for (int off = DYK_WAVE / 2; off > 0; off >>= 1) {
            a += __shfl_down(a, off);
            m = fmaxf(m, __shfl_down(m, off));
            bad += __shfl_down(bad, off);
            zer += __shfl_down(zer, off);
        }
        if (lane == 0) {
            DykTensorStat r;
            r.sumsq = a;
            r.absmax = m;
            r.nonfinite = bad > 0xffffffffull ? 0xffffffffu : (uint32_t)bad;
            r.zeros = zer > 0xffffffffull ? 0xffffffffu : (uint32_t)zer;
            r._pad = 0;
            out[(long)s * nbuf + k] = r;
        }
    }
}

template <int NBUF>
int launch_partials(const DykTensorStatsDesc* d, hipStream_t stream) {
    Bufs<NBUF> b;
    for (int k = 0; k < NBUF; ++k) b.p[k] = d->buf[k];
    hipLaunchKernelGGL(tstat_partials_kernel<NBUF>, dim3(d->nitems), dim3(kBlock), 0, stream, b, d->seg, d->items, (int)d->nseg,
                       (long)d->n, (DykTensorStat*)d->ws);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

}  // namespace

extern "C" int64_t dyk_tensor_stats_ws_bytes(int64_t nitems, int32_t nbuf) {
    if (nitems <= 0 || nitems > 0x7fffffff || nbuf < 1 || nbuf > DYK_TSTAT_MAX_BUFS) return 0;
    return (int64_t)sizeof(DykTensorStat) * nitems * nbuf;
}

extern "C" int dyk_tensor_stats(const DykTensorStatsDesc* d, void* stream) {
    if (!d || d->nbuf < 1 || d->nbuf > DYK_TSTAT_MAX_BUFS || d->nseg <= 0 || d->nitems < d->nseg) return DYK_ERR_ARG;
    if (!d->seg || !d->items || !d->ws || !d->out || d->n <= 0 || (d->n & 3)) return DYK_ERR_ARG;
    for (int k = 0; k < d->nbuf; ++k)
        if (!d->buf[k] || ((uintptr_t)d->buf[k] & 15)) return DYK_ERR_ARG;
    if (((uintptr_t)d->seg | (uintptr_t)d->items | (uintptr_t)d->ws | (uintptr_t)d->out) & 7) return DYK_ERR_ARG;
    const int64_t need = dyk_tensor_stats_ws_bytes(d->nitems, d->nbuf);
    if (need <= 0 || d->ws_bytes < need) return DYK_ERR_ARG;
    int rc;
    switch (d->nbuf) {
    case 1: rc = launch_partials<1>(d, (hipStream_t)stream); break;
    case 2: rc = launch_partials<2>(d, (hipStream_t)stream); break;
    case 3: rc = launch_partials<3>(d, (hipStream_t)stream); break;
    default: rc = launch_partials<4>(d, (hipStream_t)stream); break;
    }
    if (rc != DYK_OK) return rc;
    hipLaunchKernelGGL(tstat_fold_kernel, dim3((d->nseg + kWaves - 1) / kWaves), dim3(kBlock), 0, (hipStream_t)stream,
                       (const DykTensorStat*)d->ws, d->seg, (int)d->nseg, (int)d->nitems, (int)d->nbuf, d->out);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
