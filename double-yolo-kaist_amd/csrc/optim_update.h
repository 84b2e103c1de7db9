// The per-element statements of the fused optimizer steps, written once: adam_kernel / sgd_kernel (optim.hip), their guarded
// forms (optim_guard.hip) and the grouped kernels (optim.hip) all inline these functions, so that the same inputs and the same
// hyper-parameters give the same bits whichever entry point ran.  One call handles one 16-byte vector of p, g, m (, v).
#pragma once
#include "dyk_common.h"

namespace dyk_optim {

__device__ __forceinline__ void clear_grad_vec(const DykOptimDesc& d, long i) {
    if (d.zero_grad) ((float4*)d.g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ void store_wc_vec(const DykOptimDesc& d, long i, const float* pp) {
    if (d.wc) {
        uint2 pk;
        pk.x = (uint32_t)f32_to_bf16(pp[0]) | ((uint32_t)f32_to_bf16(pp[1]) << 16);
        pk.y = (uint32_t)f32_to_bf16(pp[2]) | ((uint32_t)f32_to_bf16(pp[3]) << 16);
        ((uint2*)d.wc)[i] = pk;
    }
}

// torch.optim.Adam with L2 weight decay; `decoupled` (torch.optim.AdamW) scales p by decay_mul first and the caller passes wd = 0
__device__ __forceinline__ void adam_vec(const DykOptimDesc& d, long i, float gs, float wd, float b1, float b2, float eps,
                                         float bc2_sqrt, float step_size, bool decoupled, float decay_mul) {
    float4 p = ((float4*)d.p)[i];
    float4 g = ((const float4*)d.g)[i];
    float4 m = ((float4*)d.m)[i];
    float4 v = ((float4*)d.v)[i];
    float* pp = (float*)&p; float* gg = (float*)&g; float* mm = (float*)&m; float* vv = (float*)&v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (decoupled) pp[j] = pp[j] * decay_mul;                 // p.mul_(1 - lr * weight_decay)
        float gr = gg[j] * gs;
        if (wd != 0.f) gr += wd * pp[j];
        mm[j] = b1 * mm[j] + (1.f - b1) * gr;                     // exp_avg.lerp_(grad, 1 - beta1)
        vv[j] = b2 * vv[j] + (1.f - b2) * gr * gr;                // exp_avg_sq
        const float denom = sqrtf(vv[j]) / bc2_sqrt + eps;
        pp[j] -= step_size * (mm[j] / denom);
    }
    ((float4*)d.p)[i] = p;
    ((float4*)d.m)[i] = m;
    ((float4*)d.v)[i] = v;
    clear_grad_vec(d, i);
    store_wc_vec(d, i, pp);
}

// torch.optim.SGD(nesterov=True, dampening=0) with L2 weight decay
__device__ __forceinline__ void sgd_vec(const DykOptimDesc& d, long i, float gs, float wd, float mom, float lr, int first_step) {
    float4 p = ((float4*)d.p)[i];
    float4 g = ((const float4*)d.g)[i];
    float4 m = ((float4*)d.m)[i];
    float* pp = (float*)&p; float* gg = (float*)&g; float* mm = (float*)&m;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float gr = gg[j] * gs;
        if (wd != 0.f) gr += wd * pp[j];
        mm[j] = first_step ? gr : mom * mm[j] + gr;               // momentum buffer (dampening 0)
        gr = gr + mom * mm[j];                                    // nesterov
        pp[j] -= lr * gr;
    }
    ((float4*)d.p)[i] = p;
    ((float4*)d.m)[i] = m;
    clear_grad_vec(d, i);
    store_wc_vec(d, i, pp);
}

}  // namespace dyk_optim
