// What the HBM-bound channels-last passes of bn_act.hip and elementwise.hip share: the strip thread mapping and its pixel walk, the
// BatchNorm arithmetic (normalise, finalize, backward terms), the replica fold and the reduce tail on the device; the descriptor
// check, the grid rule and the runtime-code -> template-argument dispatch on the host.  One loop and one formula each: a change to
// these passes is made here.
#pragma once
#include <type_traits>
#include "dyk_common.h"

// ---------------------------------------------------------------------------------------------------- the strip
// A workgroup of 256 threads is CVB channel vectors (tx) x PY = 256 / CVB pixel lanes (ty); grid.x walks channel-vector groups,
// grid.y splits the pixels into one CONTIGUOUS chunk per workgroup, a multiple of PY (round 3: with the workgroups striding over the
// whole tensor -- pixel p0 + u * gridDim.y * PY -- the 168 MB passes ran 3-6 % slower: 58.0 -> 54.7 us normalise, 102.0 -> 98.7 us
// apply on 256 x 320 x 64; C3 step -0.15 ms over four interleaved runs).  No integer division in the loop, per-channel parameters
// live in registers, and a wave touches CVB*16 contiguous bytes per pixel row (whole rows for C <= 256 bf16), i.e. fully coalesced
// when ld == C.
struct EwStrip {
    int tx, ty, c, PY, npix;    // c: first channel of this thread's vector
    bool active;                // c < C (a tail group has idle columns)
    // this thread's pixels of the workgroup's chunk: p0, p0 + PY, ... < pend
    __device__ __forceinline__ void pixels(long& p0, long& pend) const {
        const long chunk = ((npix + gridDim.y - 1) / gridDim.y + PY - 1) / PY * PY;
        pend = min((long)npix, ((long)blockIdx.y + 1) * chunk);
        p0 = (long)blockIdx.y * chunk + ty;
    }
};
template <int EPV> __device__ __forceinline__ EwStrip ew_strip(int CVB, int C, int npix) {
    EwStrip s;
    s.PY = 256 / CVB;
    s.tx = threadIdx.x % CVB;
    s.ty = threadIdx.x / CVB;
    const int cv = blockIdx.x * CVB + s.tx;
    s.c = cv * EPV;
    s.npix = npix;
    s.active = cv < C / EPV;
    return s;
}
// U pixels in flight per thread (memory-level parallelism): U guarded loads `load(p, v)` into a V each, then U times `use(p, v)`
template <int U, typename V, typename Load, typename Use> __device__ __forceinline__ void strip_walk(const EwStrip& s, Load load, Use use) {
    long first, pend;
    s.pixels(first, pend);
    const long pstep = s.PY;
    for (long p0 = first; p0 < pend; p0 += pstep * U) {
        V v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long p = p0 + u * pstep;
            if (p < pend) load(p, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long p = p0 + u * pstep;
            if (p >= pend) break;
            use(p, v[u]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- BatchNorm arithmetic
// out = act(a * sc + sh) (+ b) over the strip: the pixel loop of dyk_bn_act_fwd, with the vectors the caller holds
template <typename T, int ACT, int EPV>
__device__ __forceinline__ void bn_normalise(const EwStrip& s, const DykEwDesc& d, const float (&sc)[EPV], const float (&sh)[EPV]) {
    const int c = s.c;
    const T* __restrict__ a = (const T*)d.a;
    const T* __restrict__ r = (const T*)d.b;
    T* __restrict__ o = (T*)d.out;
    struct V { uint4 x, r; };
    strip_walk<4, V>(
        s,
        [&](long p, V& v) {
            v.x = ld_stream16(a + p * d.lda + c);
            if (r) v.r = *(const uint4*)(r + p * d.ldb + c);
        },
        [&](long p, const V& v) {
            float x[EPV], y[EPV];
            vec_unpack<T>(v.x, x);
#pragma unroll
            for (int j = 0; j < EPV; ++j) y[j] = act_fwd_c<ACT>(x[j] * sc[j] + sh[j]);
            if (r) {
                float rr[EPV];
                vec_unpack<T>(v.r, rr);
#pragma unroll
                for (int j = 0; j < EPV; ++j) y[j] += rr[j];
            }
            *(uint4*)(o + p * d.ldo + c) = vec_pack<T>(y);
        });
}

// a channel's statistics sums -> what the forward and the backward need of them (fp64 up to rstd)
struct BnAffine { double mean, var; float rstd, scale, shift; };
__device__ __forceinline__ BnAffine bn_channel_affine(double s1, double s2, double n, float eps, const float* gamma, const float* beta, int c) {
    BnAffine a;
    a.mean = s1 / n;
    a.var = s2 / n - a.mean * a.mean;
    if (a.var < 0.0) a.var = 0.0;
    a.rstd = (float)(1.0 / sqrt(a.var + (double)eps));
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;        // (null: the identity)
    a.scale = g * a.rstd;
    a.shift = b - (float)a.mean * a.scale;
    return a;
}
// scale / shift for the forward, mean / rstd for the backward, the running statistics (unbiased variance)
__device__ __forceinline__ void bn_publish(const DykBnFinalizeDesc& f, int c, const BnAffine& a, double n) {
    f.scale[c] = a.scale;
    f.shift[c] = a.shift;
    if (f.save_mean) f.save_mean[c] = (float)a.mean;
    if (f.save_rstd) f.save_rstd[c] = a.rstd;
    if (f.running_mean) {
        const double unb = n > 1.0 ? a.var * n / (n - 1.0) : a.var;
        f.running_mean[c] = (1.f - f.momentum) * f.running_mean[c] + f.momentum * (float)a.mean;
        f.running_var[c] = (1.f - f.momentum) * f.running_var[c] + f.momentum * (float)unb;
    }
}

// da = g * act'(y * sc + sh), xhat = (y - mu) * rs: what every BatchNorm-backward sum and gradient is made of (ACT < 0: runtime_act)
template <int ACT>
__device__ __forceinline__ void bn_bwd_terms(float g, float y, float sc, float sh, float mu, float rs, int runtime_act, float& da, float& xhat) {
    da = g * act_bwd_c<ACT>(y * sc + sh, runtime_act);
    xhat = (y - mu) * rs;
}

// ---------------------------------------------------------------------------------------------------- replicas
// tot[w] = sum over r < slots of p[r * stride + w * off2], both sums of a channel at once: batches of 16 replicas x 2 sums requested
// back to back -- the fold is a chain of slots / 16 dependent L2 round trips in front of the first pixel load of a launch-bound pass
// (round 3, tools/gpu_probe.py bnfold: 32 replicas in batches of 4 cost 3.5 us of a 10 us launch on the 32 x 40 x 256 tensors, 1
// replica 0 us; the backward's 16 replicas as a dependent chain ~10 us) -- into NACC accumulators each, then batches of NACC, then
// singles into the first, then a pairwise tree
template <int NACC> __device__ __forceinline__ void fold_replicas(const double* p, size_t stride, size_t off2, int slots_or_0, double (&tot)[2]) {
    constexpr int FB = 16;
    const int slots = slots_or_0 > 0 ? slots_or_0 : 1;
    double acc[2][NACC];
#pragma unroll
    for (int u = 0; u < NACC; ++u) acc[0][u] = acc[1][u] = 0.0;
    int r = 0;
    for (; r + FB <= slots; r += FB) {
        double v[2][FB];
#pragma unroll
        for (int u = 0; u < FB; ++u) { v[0][u] = p[(size_t)(r + u) * stride]; v[1][u] = p[(size_t)(r + u) * stride + off2]; }
#pragma unroll
        for (int u = 0; u < FB; ++u) { acc[0][u & (NACC - 1)] += v[0][u]; acc[1][u & (NACC - 1)] += v[1][u]; }
    }
    for (; r + NACC <= slots; r += NACC) {
#pragma unroll
        for (int u = 0; u < NACC; ++u) { acc[0][u] += p[(size_t)(r + u) * stride]; acc[1][u] += p[(size_t)(r + u) * stride + off2]; }
    }
    for (; r < slots; ++r) { acc[0][0] += p[(size_t)r * stride]; acc[1][0] += p[(size_t)r * stride + off2]; }
#pragma unroll
    for (int w = NACC / 2; w > 0; w >>= 1) {
#pragma unroll
        for (int i = 0; i < w; ++i) { acc[0][i] = acc[0][2 * i] + acc[0][2 * i + 1]; acc[1][i] = acc[1][2 * i] + acc[1][2 * i + 1]; }
    }
    tot[0] = acc[0][0];
    tot[1] = acc[1][0];
}

// the NS partial sums of every thread through LDS (red: 256 * NS * 8 floats), folded over ty in lane order q = 1 .. PY - 1 by the
// threads of pixel lane 0; true for the threads that then hold their channels' sums of the workgroup
template <int NS, int EPV>
__device__ __forceinline__ bool strip_fold(float* red, float (&s)[NS][EPV], int CVB, int PY, int tx, int ty, bool active) {
    float* mine = red + threadIdx.x * NS * 8;
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
#pragma unroll
        for (int n = 0; n < NS; ++n) mine[n * 8 + j] = s[n][j];
    }
    __syncthreads();
    if (ty != 0 || !active) return false;
    for (int q = 1; q < PY; ++q) {
        const float* o = red + (q * CVB + tx) * NS * 8;
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
#pragma unroll
            for (int n = 0; n < NS; ++n) s[n][j] += o[n * 8 + j];
        }
    }
    return true;
}
// one fp64 atomic per channel and sum into replica index % slots of red [slots][2][C]
template <int EPV> __device__ __forceinline__ void replica_atomics(double* red, int C, int c, unsigned index, int slots, const float (&s)[2][EPV]) {
    double* rd = red + (size_t)(index % (unsigned)(slots > 0 ? slots : 1)) * 2 * C;
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
        atomicAdd(rd + c + j, (double)s[0][j]);
        atomicAdd(rd + C + c + j, (double)s[1][j]);
    }
}

// ---------------------------------------------------------------------------------------------------- the host side
inline int ew_epv(int dtype) { return dtype == DYK_F32 ? 4 : 8; }

// the operands every elementwise launcher needs: a, the storage type, C and the row strides in whole 16-byte vectors.  Two-problem
// launches (DykEwDesc.twin) are for the BatchNorm passes and axpby only.
inline int ew_check(const DykEwDesc* d, bool need_out, bool need_b, bool twin_ok, bool need_npix) {
    if (!d || !d->a || (need_out && !d->out) || (need_b && !d->b)) return DYK_ERR_ARG;
    if (d->twin && !twin_ok) return DYK_ERR_UNSUPPORTED;
    if (d->dtype != DYK_BF16 && d->dtype != DYK_F32 && d->dtype != DYK_F16) return DYK_ERR_ARG;
    const int epv = ew_epv(d->dtype);
    if ((need_npix && d->npix <= 0) || d->C <= 0 || d->C % epv || d->lda % epv || (need_out && d->ldo % epv) || (d->b && d->ldb % epv))
        return DYK_ERR_ARG;
    return DYK_OK;
}

// grid of the strip mapping over CV channel vectors x npix pixels, at most cap_wgs workgroups: returns CVB, fills gx / gy
inline int ew_grid2d(int CV, long npix, long cap_wgs, int* gx, int* gy) {
    int CVB = 1;
    while (CVB < CV && CVB < 32) CVB <<= 1;
    const int PY = 256 / CVB;
    *gx = (CV + CVB - 1) / CVB;
    constexpr int ppt = 8;                                      // (4 / 16 pixels per thread, grid caps 1 024 / 4 096: +-0.2 ms, round 2)
    long g = (npix + (long)PY * ppt - 1) / ((long)PY * ppt);    // >= 8 pixels per thread (2 unrolled iterations)
    const long cap = cap_wgs / *gx > 0 ? cap_wgs / *gx : 1;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    *gy = (int)g;
    return CVB;
}

// A runtime code becomes a template argument on the host, so that the kernels' inner loops are branch-free.
// ew_launch_dtype: f(EwType<T>()) launches the instantiation for the storage type, then the launch check.  f16 is the inference type
// (forward kernels only): where F16_OK is false it has no kernel -- DYK_ERR_UNSUPPORTED and no instantiation.
template <typename T> struct EwType { typedef T type; };
template <typename Tag> using ew_t = typename Tag::type;
template <bool F16_OK, typename F> inline int ew_launch_dtype(int dtype, F&& f) {
    if (dtype == DYK_F16) {
        if constexpr (F16_OK) f(EwType<f16_t>());
        else return DYK_ERR_UNSUPPORTED;
    } else if (dtype == DYK_BF16) f(EwType<bf16_t>());
    else if (dtype == DYK_F32) f(EwType<float>());
    else return DYK_ERR_ARG;
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
// ew_dispatch_int: f(integral_constant<int, V>()) for the V of the list that equals v; false (and no call) when none does
template <int... V> struct EwInts {};
typedef EwInts<DYK_ACT_LINEAR, DYK_ACT_LEAKY, DYK_ACT_MISH, DYK_ACT_RELU, DYK_ACT_RELU6, DYK_ACT_HSIGMOID, DYK_ACT_HSWISH> EwAllActs;
template <typename F, int V0, int... V> inline bool ew_dispatch_int(int v, EwInts<V0, V...>, F&& f) {
    if (v == V0) { f(std::integral_constant<int, V0>()); return true; }
    if constexpr (sizeof...(V) > 0) return ew_dispatch_int(v, EwInts<V...>(), f);
    else return false;
}
