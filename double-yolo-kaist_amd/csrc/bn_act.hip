// BatchNorm2d (train-mode batch statistics) + activation, forward and backward.  All HBM-bound
// channels-last kernels, 16-byte vectors, per-channel parameters in fp32, cross-block
// reductions in fp64 atomics.
//
// Forward of nn.Sequential(Conv2d, BatchNorm2d, act) (reference models.py:34-62) in training:
//   conv kernel (raw output + per-channel sum / sum^2)  ->  dyk_bn_finalize  ->  dyk_bn_act_fwd
// Backward:
//   dyk_bn_act_bwd_reduce (sum dact, sum dact*xhat) -> dyk_bn_bwd_params (dgamma, dbeta)
//   -> dyk_bn_act_bwd_apply (gradient w.r.t. the raw conv output) -> conv dgrad / wgrad.
//
// ew_strip.h holds what these passes share with each other and with the squeeze-excitation passes of elementwise.hip: the strip
// thread mapping and its pixel walk (EwStrip, strip_walk), the arithmetic (bn_normalise, bn_channel_affine / bn_publish, bn_bwd_terms),
// the replica fold (fold_replicas), the reduce tail (strip_fold, replica_atomics) and the launchers' descriptor check, grid rule and
// dtype / activation dispatch.
#include <stdlib.h>
#include "ew_strip.h"

namespace {

// 32 lanes per channel: lane r sums replicas r, r+32, ... , a 5-step xor-shuffle folds them, lane 0 finalises
__global__ __launch_bounds__(256) void bn_finalize_kernel(DykFinPair pr) {
    const DykBnFinalizeDesc d = pr.d[blockIdx.z];
    const int sub = threadIdx.x & 31;
    const int c = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    if (c >= d.C) return;
    const double n = (double)d.count;
    const int slots = d.slots > 0 ? d.slots : 1;
    double s1 = 0.0, s2 = 0.0;
    for (int r = sub; r < slots; r += 32) {
        double* st = d.stats + (size_t)r * 2 * d.C;
        s1 += st[c]; s2 += st[d.C + c];
        st[c] = 0.0; st[d.C + c] = 0.0;          // re-arm the accumulators for the next step
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if (sub != 0) return;
    bn_publish(d, c, bn_channel_affine(s1, s2, n, d.eps, d.gamma, d.beta, c), n);
}

// eval-mode BN folded to scale/shift: scale = gamma / sqrt(running_var + eps)
__global__ void bn_fold_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                               float* scale, float* shift, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float sc = (gamma ? gamma[c] : 1.f) / sqrtf(rv[c] + eps);
    scale[c] = sc;
    shift[c] = (beta ? beta[c] : 0.f) - rm[c] * sc;
}

template <typename T, int ACT>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(DykEwPair pr, int CVB) {
    const DykEwDesc d = pr.d[blockIdx.z];          // a COPY, not a reference (see DykEwPair in dyk_common.h)
    constexpr int EPV = ElemTraits<T>::EPV;
    const EwStrip s = ew_strip<EPV>(CVB, d.C, d.npix);
    if (!s.active) return;
    float sc[EPV], sh[EPV];
#pragma unroll
    for (int j = 0; j < EPV; ++j) { sc[j] = d.p0 ? d.p0[s.c + j] : 1.f; sh[j] = d.p1 ? d.p1[s.c + j] : 0.f; }
    bn_normalise<T, ACT>(s, d, sc, sh);
}

// bn_finalize + bn_act_fwd in one launch (the 7 us finalize launch sat on the critical chain of the forward pass):
// every workgroup folds the statistics replicas of its own <= 256 channels, derives scale / shift into LDS, and the
// workgroups of grid row 0 also publish scale / shift / mean / rstd for the backward pass and update the running
// statistics.  The replicas are NOT re-armed here (other workgroups may still be reading them): the caller zeroes the
// statistics arena once per forward pass.
template <typename T, int ACT>
__global__ __launch_bounds__(256) void bn_fused_fwd_kernel(DykFinPair fp, DykEwPair pr, int CVB) {
    const DykBnFinalizeDesc f = fp.d[blockIdx.z];
    const DykEwDesc d = pr.d[blockIdx.z];          // a COPY, not a reference (see DykEwPair in dyk_common.h)
    constexpr int EPV = ElemTraits<T>::EPV;
    __shared__ float s_aff[2][256];
    {
        const int c_base = blockIdx.x * CVB * EPV;
        const int nch = min(CVB * EPV, d.C - c_base);
        for (int cl = threadIdx.x; cl < nch; cl += 256) {
            const int c = c_base + cl;
            double tot[2];
            fold_replicas<4>(f.stats + c, (size_t)2 * f.C, (size_t)f.C, f.slots, tot);
            const double n = (double)f.count;
            const BnAffine a = bn_channel_affine(tot[0], tot[1], n, f.eps, f.gamma, f.beta, c);
            s_aff[0][cl] = a.scale;
            s_aff[1][cl] = a.shift;
            if (blockIdx.y == 0) bn_publish(f, c, a, n);
        }
        __syncthreads();
    }
    const EwStrip s = ew_strip<EPV>(CVB, d.C, d.npix);
    if (!s.active) return;
    float sc[EPV], sh[EPV];
#pragma unroll
    for (int j = 0; j < EPV; ++j) { sc[j] = s_aff[0][s.tx * EPV + j]; sh[j] = s_aff[1][s.tx * EPV + j]; }
    bn_normalise<T, ACT>(s, d, sc, sh);
}

template <typename T, int ACT>
__global__ __launch_bounds__(256) void bn_act_bwd_reduce_kernel(DykEwPair pr, int CVB) {
    const DykEwDesc d = pr.d[blockIdx.z];          // a COPY, not a reference (see DykEwPair in dyk_common.h)
    constexpr int EPV = ElemTraits<T>::EPV;
    __shared__ float red[256 * 2 * 8];
    const EwStrip s = ew_strip<EPV>(CVB, d.C, d.npix);
    float sum[2][EPV];                             // sum(da), sum(da * xhat)
#pragma unroll
    for (int j = 0; j < EPV; ++j) sum[0][j] = sum[1][j] = 0.f;
    if (s.active) {
        const int c = s.c;
        float sc[EPV], sh[EPV], mu[EPV], rs[EPV];
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
            sc[j] = d.p0[c + j]; sh[j] = d.p1[c + j]; mu[j] = d.p2[c + j]; rs[j] = d.p3[c + j];
        }
        const T* __restrict__ dz = (const T*)d.a;
        const T* __restrict__ y = (const T*)d.b;
        struct V { uint4 g, y; };
        strip_walk<4, V>(
            s, [&](long p, V& v) { v.g = ld_stream16(dz + p * d.lda + c); v.y = ld_stream16(y + p * d.ldb + c); },
            [&](long, const V& v) {
                float g[EPV], yy[EPV];
                vec_unpack<T>(v.g, g);
                vec_unpack<T>(v.y, yy);
#pragma unroll
                for (int j = 0; j < EPV; ++j) {
                    float da, xh;
                    bn_bwd_terms<ACT>(g[j], yy[j], sc[j], sh[j], mu[j], rs[j], 0, da, xh);
                    sum[0][j] += da;
                    sum[1][j] += da * xh;
                }
            });
    }
    if (strip_fold<2>(red, sum, CVB, s.PY, s.tx, s.ty, s.active)) replica_atomics(d.red, d.C, s.c, blockIdx.y, d.slots, sum);
}

__global__ __launch_bounds__(256) void bn_bwd_params_kernel(double* red, float* dgamma, float* dbeta, int C, int slots) {
    const int sub = threadIdx.x & 31;
    const int c = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int r = sub; r < slots; r += 32) { s1 += red[(size_t)r * 2 * C + c]; s2 += red[(size_t)r * 2 * C + C + c]; }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if (sub != 0) return;
    red[c] = s1; red[C + c] = s2;            // replica 0 now holds the totals (read by the apply kernel)
    if (dbeta) dbeta[c] += (float)s1;
    if (dgamma) dgamma[c] += (float)s2;
}

// The totals of the reduce pass are folded here (every workgroup sums the `slots` replicas of its own <= 256
// channels), and the workgroups of grid row 0 add them to dgamma / dbeta (aux / aux2): no separate
// parameter-gradient launch on the critical chain of the backward pass.
template <typename T, int ACT>
__global__ __launch_bounds__(256) void bn_act_bwd_apply_kernel(DykEwPair pr, int CVB) {
    const DykEwDesc d = pr.d[blockIdx.z];          // a COPY, not a reference (see DykEwPair in dyk_common.h)
    constexpr int EPV = ElemTraits<T>::EPV;
    __shared__ float s_tot[2][256];
    {
        const int c_base = blockIdx.x * CVB * EPV;
        const int nch = min(CVB * EPV, d.C - c_base);
        // replicas [slots][2][C] of this layer's own reduction -- or columns of a wider one (the joint reduction over the
        // sections a [route] concatenates, DYK_EPI_BNBWD of the route's reader): H = replica stride, W = offset of the second sum
        const size_t rs = d.H > 0 ? (size_t)d.H : (size_t)2 * d.C;
        const size_t so = d.W > 0 ? (size_t)d.W : (size_t)d.C;
        for (int cl = threadIdx.x; cl < nch; cl += 256) {
            double tot[2];
            fold_replicas<8>(d.red + c_base + cl, rs, so, d.slots, tot);
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                s_tot[which][cl] = (float)tot[which];
                if (blockIdx.y == 0) {
                    float* g = which ? (float*)d.aux : (float*)d.aux2;      // sum(dact * xhat) -> dgamma, sum(dact) -> dbeta
                    if (g) g[c_base + cl] += (float)tot[which];
                }
            }
        }
        __syncthreads();
    }
    const EwStrip s = ew_strip<EPV>(CVB, d.C, d.npix);
    if (!s.active) return;
    const int c = s.c;
    const float invn = 1.f / (float)d.npix;
    float sc[EPV], sh[EPV], mu[EPV], rs[EPV], m1[EPV], m2[EPV];
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
        sc[j] = d.p0[c + j]; sh[j] = d.p1[c + j]; mu[j] = d.p2[c + j]; rs[j] = d.p3[c + j];
        m1[j] = s_tot[0][s.tx * EPV + j] * invn; m2[j] = s_tot[1][s.tx * EPV + j] * invn;
    }
    const T* __restrict__ dz = (const T*)d.a;
    const T* __restrict__ y = (const T*)d.b;
    T* __restrict__ o = (T*)d.out;
    const bool accum = d.flags & DYK_EW_ACCUM;
    struct V { uint4 g, y, o; };
    strip_walk<4, V>(
        s,
        [&](long p, V& v) {
            v.g = ld_stream16(dz + p * d.lda + c);
            v.y = ld_stream16(y + p * d.ldb + c);
            if (accum) v.o = *(const uint4*)(o + p * d.ldo + c);
        },
        [&](long p, const V& v) {
            float g[EPV], yy[EPV], r[EPV];
            vec_unpack<T>(v.g, g);
            vec_unpack<T>(v.y, yy);
#pragma unroll
            for (int j = 0; j < EPV; ++j) {
                float da, xh;
                bn_bwd_terms<ACT>(g[j], yy[j], sc[j], sh[j], mu[j], rs[j], 0, da, xh);
                r[j] = sc[j] * (da - m1[j] - xh * m2[j]);      // sc = gamma * rstd
            }
            if (accum) {
                float old[EPV];
                vec_unpack<T>(v.o, old);
#pragma unroll
                for (int j = 0; j < EPV; ++j) r[j] += old[j];
            }
            *(uint4*)(o + p * d.ldo + c) = vec_pack<T>(r);
        });
}

// one instantiation per (element type, activation): both switches are resolved on the host, launch(EwType<T>, integral_constant<ACT>).
// F16_OK: the forward pass an inference plan issues; the training passes are bf16 | f32 (f16: DYK_ERR_UNSUPPORTED).  An activation
// code outside the seven: DYK_ERR_ARG.
template <bool F16_OK, typename Launch> int bn_launch(const DykEwDesc* d, Launch launch) {
    bool known_act = false;
    const int rc = ew_launch_dtype<F16_OK>(d->dtype, [&](auto t) { known_act = ew_dispatch_int(d->act, EwAllActs(), [&](auto a) { launch(t, a); }); });
    return rc ? rc : (known_act ? DYK_OK : DYK_ERR_ARG);
}

// the strip grid of a BatchNorm pass: at most 2048 workgroups
inline int bn_grid(const DykEwDesc* d, int* gx, int* gy) { return ew_grid2d(d->C / ew_epv(d->dtype), d->npix, 2048, gx, gy); }

inline bool fin_ok(const DykBnFinalizeDesc* f) { return f && f->stats && f->scale && f->shift && f->C > 0 && f->count > 0; }

}  // namespace

extern "C" int dyk_bn_finalize(const DykBnFinalizeDesc* d, void* stream) {
    if (!fin_ok(d)) return DYK_ERR_ARG;
    DykFinPair fp;
    const int nz = dyk_fill_fin_pair(fp, d);
    if (!nz) return DYK_ERR_ARG;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((d->C + 7) / 8, 1, nz), dim3(256), 0, (hipStream_t)stream, fp);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, float eps, float* scale, float* shift, int32_t C,
                           void* stream) {
    if (!running_mean || !running_var || !scale || !shift || C <= 0) return DYK_ERR_ARG;
    hipLaunchKernelGGL(bn_fold_kernel, dim3((C + 127) / 128), dim3(128), 0, (hipStream_t)stream, gamma, beta,
                       running_mean, running_var, eps, scale, shift, C);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_bn_act_fwd(const DykEwDesc* d, void* stream) {
    const int rc = ew_check(d, true, false, true, true);
    if (rc) return rc;
    int gx, gy;
    const int CVB = bn_grid(d, &gx, &gy);
    DykEwPair pr;
    const int nz = dyk_fill_ew_pair(pr, d);
    if (!nz) return DYK_ERR_ARG;
    return bn_launch<true>(d, [&](auto t, auto a) {
        hipLaunchKernelGGL((bn_act_fwd_kernel<ew_t<decltype(t)>, decltype(a)::value>), dim3(gx, gy, nz), dim3(256), 0, (hipStream_t)stream, pr, CVB);
    });
}

extern "C" int dyk_bn_finalize_act_fwd(const DykBnFinalizeDesc* f, const DykEwDesc* d, void* stream) {
    if (!fin_ok(f)) return DYK_ERR_ARG;
    const int rc = ew_check(d, true, false, true, true);
    if (rc) return rc;
    if (d->C != f->C) return DYK_ERR_ARG;
    int gx, gy;
    const int CVB = bn_grid(d, &gx, &gy);
    DykEwPair pr;
    DykFinPair fp;
    const int nz = dyk_fill_ew_pair(pr, d);
    if (!nz || dyk_fill_fin_pair(fp, f) != nz) return DYK_ERR_ARG;       // both descriptors paired, or neither
    return bn_launch<false>(d, [&](auto t, auto a) {
        hipLaunchKernelGGL((bn_fused_fwd_kernel<ew_t<decltype(t)>, decltype(a)::value>), dim3(gx, gy, nz), dim3(256), 0, (hipStream_t)stream, fp, pr, CVB);
    });
}

extern "C" int dyk_bn_act_bwd_reduce(const DykEwDesc* d, void* stream) {
    if (!d || !d->a || !d->b || !d->red || !d->p0 || !d->p1 || !d->p2 || !d->p3) return DYK_ERR_ARG;
    if (d->dtype == DYK_F16) return DYK_ERR_UNSUPPORTED;       // (the inference type has no backward forms)
    const int rc = ew_check(d, false, true, true, true);
    if (rc) return rc;
    int gx, gy;
    const int CVB = bn_grid(d, &gx, &gy);
    DykEwPair pr;
    const int nz = dyk_fill_ew_pair(pr, d);
    if (!nz) return DYK_ERR_ARG;
    return bn_launch<false>(d, [&](auto t, auto a) {
        hipLaunchKernelGGL((bn_act_bwd_reduce_kernel<ew_t<decltype(t)>, decltype(a)::value>), dim3(gx, gy, nz), dim3(256), 0, (hipStream_t)stream, pr, CVB);
    });
}

extern "C" int dyk_bn_bwd_params(double* red, float* dgamma, float* dbeta, int32_t C, int32_t slots, void* stream) {
    if (!red || C <= 0) return DYK_ERR_ARG;
    hipLaunchKernelGGL(bn_bwd_params_kernel, dim3((C + 7) / 8), dim3(256), 0, (hipStream_t)stream, red, dgamma, dbeta, C,
                       slots > 0 ? slots : 1);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_bn_act_bwd_apply(const DykEwDesc* d, void* stream) {
    const int rc = ew_check(d, true, true, true, true);
    if (rc) return rc;
    if (d->flags & DYK_EW_SKIP) return DYK_OK;          // done inside the consumer (DykStemDesc.bn_fused)
    if (!d->red || !d->p0 || !d->p1 || !d->p2 || !d->p3) return DYK_ERR_ARG;
    int gx, gy;
    const int CVB = bn_grid(d, &gx, &gy);
    DykEwPair pr;
    const int nz = dyk_fill_ew_pair(pr, d);
    if (!nz) return DYK_ERR_ARG;
    return bn_launch<false>(d, [&](auto t, auto a) {
        hipLaunchKernelGGL((bn_act_bwd_apply_kernel<ew_t<decltype(t)>, decltype(a)::value>), dim3(gx, gy, nz), dim3(256), 0, (hipStream_t)stream, pr, CVB);
    });
}
