// Exponential moving average of the flat parameter / running-statistics buffers (ModelEMA.update, reference
// build_utils/torch_utils.py:77-126): one launch for every floating state_dict entry of the model instead of ~3 torch
// kernels per entry.  Per element, exactly what torch computes for `v *= d; v += (1. - d) * m` on fp32 tensors:
//     dst = fl32(fl32(dst * d) + fl32(omd * src))          (d = fl32(decay), omd = fl32(1 - decay) formed in double)
// The products and the sum are separate IEEE operations: the Makefile builds with -ffp-contract=on, and an FMA would round
// once instead of twice (not bit-identical to torch).  HBM-bound: 16-byte vectors, grid-stride loop.
#include "dyk_common.h"

namespace {

__device__ __forceinline__ float ema1(float v, float m, float d, float omd) {
    return __fadd_rn(__fmul_rn(v, d), __fmul_rn(omd, m));
}

__global__ __launch_bounds__(256) void ema_kernel(DykEmaDesc e) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long first = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const float d = e.d, omd = e.omd;
    for (int r = 0; r < e.nregions; ++r) {                       // regions back to back: no thread waits for the largest
        const float4* src = (const float4*)e.src[r];
        float4* dst = (float4*)e.dst[r];
        const long n4 = e.n[r] >> 2;
        for (long i = first; i < n4; i += stride) {
            const float4 m = src[i];
            float4 v = dst[i];
            v.x = ema1(v.x, m.x, d, omd);
            v.y = ema1(v.y, m.y, d, omd);
            v.z = ema1(v.z, m.z, d, omd);
            v.w = ema1(v.w, m.w, d, omd);
            dst[i] = v;
        }
    }
}

}  // namespace

extern "C" int dyk_ema_update(const DykEmaDesc* e, void* stream) {
    if (!e || e->nregions < 1 || e->nregions > DYK_EMA_MAX_REGIONS) return DYK_ERR_ARG;
    long most = 0;
    for (int r = 0; r < e->nregions; ++r) {
        if (!e->src[r] || !e->dst[r] || e->n[r] <= 0 || (e->n[r] & 3)) return DYK_ERR_ARG;
        if (((uintptr_t)e->src[r] | (uintptr_t)e->dst[r]) & 15) return DYK_ERR_ARG;
        if (e->n[r] > most) most = e->n[r];
    }
    long g = ((most >> 2) + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(ema_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, *e);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
