// Fused optimizer steps over the flat parameter / gradient buffers (one launch for all 116 M
// parameters): Adam and SGD-Nesterov with L2 weight decay exactly as torch.optim applies them
// (reference train.py:85-91 builds optim.Adam / optim.SGD over one parameter group), optional
// gradient scaling (1/world_size, loss-scale removal), optional emission of the compute-dtype weight
// copy and optional zeroing of the gradient for the next accumulation.  HBM-bound: 16-byte vectors.
// The per-element statements live in optim_update.h; the grouped kernels below (parameter groups, decoupled weight decay)
// and the guarded ones of optim_guard.hip share them.
#include <math.h>
#include "dyk_common.h"
#include "optim_update.h"

namespace {

// the mask word of vector i: 0 = frozen parameters (entries are 64-element aligned, so the four bytes agree)
__device__ __forceinline__ uint32_t mask_word(const DykOptimDesc& d, long i) { return ((const uint32_t*)d.mask)[i]; }

__global__ __launch_bounds__(256) void adam_kernel(DykOptimDesc d, float bc1, float bc2_sqrt) {
    const long n4 = d.n >> 2;
    const float lr = d.lr, b1 = d.beta1, b2 = d.beta2, eps = d.eps, wd = d.weight_decay, gs = d.grad_scale;
    const float step_size = lr / bc1;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        if (d.mask && mask_word(d, i) == 0) {
            dyk_optim::clear_grad_vec(d, i);
            continue;
        }
        dyk_optim::adam_vec(d, i, gs, wd, b1, b2, eps, bc2_sqrt, step_size, false, 1.f);
    }
}

__global__ __launch_bounds__(256) void sgd_kernel(DykOptimDesc d, int first_step) {
    const long n4 = d.n >> 2;
    const float lr = d.lr, mom = d.beta1, wd = d.weight_decay, gs = d.grad_scale;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        if (d.mask && mask_word(d, i) == 0) {
            dyk_optim::clear_grad_vec(d, i);
            continue;
        }
        dyk_optim::sgd_vec(d, i, gs, wd, mom, lr, first_step);
    }
}

// ---- parameter groups: the mask byte names the group (include/dyk_hip.h).  The table arrives as a kernel argument; every
// workgroup turns it into one 16-byte record per group in LDS ({step_size | lr, wd, decay_mul, flags}, slot 0 = frozen) that a
// lane reads with the byte of its vector -- a wave spans 256 elements, i.e. up to four groups.
struct GroupRec {
    float a, wd, decay_mul;
    uint32_t flags;
};

__global__ __launch_bounds__(256) void adam_groups_kernel(DykOptimDesc d, DykOptimGroups gr, const DykGradGuardRec* __restrict__ rec,
                                                          float bc1, float bc2_sqrt) {
    const long n4 = d.n >> 2;
    float gs = d.grad_scale;
    if (rec) {
        if (rec->skip) {
            for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
                dyk_optim::clear_grad_vec(d, i);
            return;
        }
        bc1 = rec->bc1;
        bc2_sqrt = rec->bc2_sqrt;
        gs = __fmul_rn(d.grad_scale, rec->coef);
    }
    __shared__ GroupRec tab[DYK_OPT_MAX_GROUPS + 1];
    if (threadIdx.x <= DYK_OPT_MAX_GROUPS) {
        GroupRec r = {0.f, 0.f, 1.f, 0u};
        if (threadIdx.x >= 1 && (int)threadIdx.x <= gr.count) {
            const DykOptimGroup g = gr.g[threadIdx.x - 1];
            const bool dec = (g.flags & DYK_OPT_GROUP_DECOUPLED) != 0;
            r.a = g.lr / bc1;                                     // step_size, as adam_kernel forms it
            r.wd = dec ? 0.f : g.weight_decay;
            r.decay_mul = g.decay_mul;
            r.flags = g.flags;
        }
        tab[threadIdx.x] = r;
    }
    __syncthreads();
    const uint32_t count = (uint32_t)gr.count;
    const float b1 = d.beta1, b2 = d.beta2, eps = d.eps;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const uint32_t k = mask_word(d, i) & 0xffu;
        if (k == 0 || k > count) {
            dyk_optim::clear_grad_vec(d, i);
            continue;
        }
        const GroupRec r = tab[k];
        dyk_optim::adam_vec(d, i, gs, r.wd, b1, b2, eps, bc2_sqrt, r.a, (r.flags & DYK_OPT_GROUP_DECOUPLED) != 0, r.decay_mul);
    }
}

__global__ __launch_bounds__(256) void sgd_groups_kernel(DykOptimDesc d, DykOptimGroups gr, const DykGradGuardRec* __restrict__ rec,
                                                         int first_step) {
    const long n4 = d.n >> 2;
    float gs = d.grad_scale;
    if (rec) {
        if (rec->skip) {
            for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
                dyk_optim::clear_grad_vec(d, i);
            return;
        }
        first_step = rec->applied == 1 ? 1 : 0;
        gs = __fmul_rn(d.grad_scale, rec->coef);
    }
    __shared__ GroupRec tab[DYK_OPT_MAX_GROUPS + 1];
    if (threadIdx.x <= DYK_OPT_MAX_GROUPS) {
        GroupRec r = {0.f, 0.f, 1.f, 0u};
        if (threadIdx.x >= 1 && (int)threadIdx.x <= gr.count) {
            const DykOptimGroup g = gr.g[threadIdx.x - 1];
            r.a = g.lr;
            r.wd = g.weight_decay;
        }
        tab[threadIdx.x] = r;
    }
    __syncthreads();
    const uint32_t count = (uint32_t)gr.count;
    const float mom = d.beta1;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const uint32_t k = mask_word(d, i) & 0xffu;
        if (k == 0 || k > count) {
            dyk_optim::clear_grad_vec(d, i);
            continue;
        }
        const GroupRec r = tab[k];
        dyk_optim::sgd_vec(d, i, gs, r.wd, mom, r.a, first_step);
    }
}

int check(const DykOptimDesc* d, bool need_v) {
    if (!d || !d->p || !d->g || !d->m || (need_v && !d->v) || d->n <= 0 || (d->n & 3)) return DYK_ERR_ARG;
    if (((uintptr_t)d->p | (uintptr_t)d->g | (uintptr_t)d->m | (uintptr_t)d->v) & 15) return DYK_ERR_ARG;
    if (d->wc && ((uintptr_t)d->wc & 7)) return DYK_ERR_ARG;
    if (d->mask && ((uintptr_t)d->mask & 3)) return DYK_ERR_ARG;
    return DYK_OK;
}

// the checks of the grouped entries that go beyond check(): DYK_OK, DYK_ERR_ARG, or DYK_ERR_UNSUPPORTED for a decoupled group
// where `allow_decoupled` is false (a bad argument anywhere wins over that)
int check_groups(const DykOptimDesc* d, const DykOptimGroups* gr, const DykGradGuardRec* rec, bool allow_decoupled) {
    if (!gr || !d->mask) return DYK_ERR_ARG;
    if (gr->count < 1 || gr->count > DYK_OPT_MAX_GROUPS) return DYK_ERR_ARG;
    if (rec ? ((uintptr_t)rec & 7) != 0 : d->step <= 0) return DYK_ERR_ARG;
    bool decoupled = false;
    for (int k = 0; k < gr->count; ++k) {
        const DykOptimGroup& g = gr->g[k];
        if (!isfinite(g.lr) || !(g.weight_decay >= 0.f) || (g.flags & ~(uint32_t)DYK_OPT_GROUP_DECOUPLED)) return DYK_ERR_ARG;
        decoupled |= (g.flags & DYK_OPT_GROUP_DECOUPLED) != 0;
    }
    return (decoupled && !allow_decoupled) ? DYK_ERR_UNSUPPORTED : DYK_OK;
}

long step_grid(long n) {
    long g = ((n >> 2) + 255) / 256;
    return g > 8192 ? 8192 : g;
}

}  // namespace

extern "C" int dyk_adam_step(const DykOptimDesc* d, void* stream) {
    const int rc = check(d, true);
    if (rc) return rc;
    if (d->step <= 0) return DYK_ERR_ARG;
    const double bc1 = 1.0 - pow((double)d->beta1, (double)d->step);
    const double bc2 = 1.0 - pow((double)d->beta2, (double)d->step);
    long g = ((d->n >> 2) + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(adam_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, *d, (float)bc1, (float)sqrt(bc2));
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_sgd_step(const DykOptimDesc* d, void* stream) {
    const int rc = check(d, false);
    if (rc) return rc;
    if (d->step <= 0) return DYK_ERR_ARG;
    long g = ((d->n >> 2) + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(sgd_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, *d, d->step == 1 ? 1 : 0);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_adam_step_groups(const DykOptimDesc* d, const DykOptimGroups* gr, const DykGradGuardRec* rec, void* stream) {
    int rc = check(d, true);
    if (rc) return rc;
    rc = check_groups(d, gr, rec, true);
    if (rc) return rc;
    float bc1 = 0.f, bc2_sqrt = 0.f;                              // (read from the record when there is one)
    if (!rec) {
        bc1 = (float)(1.0 - pow((double)d->beta1, (double)d->step));
        bc2_sqrt = (float)sqrt(1.0 - pow((double)d->beta2, (double)d->step));
    }
    hipLaunchKernelGGL(adam_groups_kernel, dim3((int)step_grid(d->n)), dim3(256), 0, (hipStream_t)stream, *d, *gr, rec, bc1, bc2_sqrt);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int dyk_sgd_step_groups(const DykOptimDesc* d, const DykOptimGroups* gr, const DykGradGuardRec* rec, void* stream) {
    int rc = check(d, false);
    if (rc) return rc;
    rc = check_groups(d, gr, rec, false);
    if (rc) return rc;
    hipLaunchKernelGGL(sgd_groups_kernel, dim3((int)step_grid(d->n)), dim3(256), 0, (hipStream_t)stream, *d, *gr, rec,
                       (!rec && d->step == 1) ? 1 : 0);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
