// Fused optimizer steps over the flat parameter / gradient buffers (one launch for all 116 M
// parameters): Adam and SGD-Nesterov with L2 weight decay exactly as torch.optim applies them
// (reference train.py:85-91 builds optim.Adam / optim.SGD over one parameter group), optional
// gradient scaling (1/world_size, loss-scale removal), optional emission of the compute-dtype weight
// copy and optional zeroing of the gradient for the next accumulation.  HBM-bound: 16-byte vectors.
// One kernel template over (update rule, parameter groups or not, record possible or not) serves the six entry points: the plain ones, the _guarded
// ones (skip / clip coefficient / bias corrections from the record that dyk_grad_stats of optim_guard.hip leaves) and the
// _groups ones (per-group lr / weight decay, decoupled weight decay).  The per-element statements are written once, so the same
// inputs and the same hyper-parameters give the same bits whichever entry point ran.
#include <math.h>
#include <type_traits>
#include "dyk_common.h"

namespace {

// ---- the per-element statements: one call handles one 16-byte vector of p, g, m (, v)
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

// ---- the step kernel
enum class Rule { Adam, Sgd };

struct NoGroups {};              // the table of the ungrouped instantiations: d.lr / d.weight_decay hold for every live element

// what a live element needs from its group: {step_size | lr, wd, decay_mul, flags}
struct GroupRec {
    float a, wd, decay_mul;
    uint32_t flags;
};

template <Rule R>
__device__ __forceinline__ GroupRec group_rec(float lr, float weight_decay, float decay_mul, uint32_t flags, float bc1) {
    if constexpr (R == Rule::Adam)
        return {lr / bc1, (flags & DYK_OPT_GROUP_DECOUPLED) ? 0.f : weight_decay, decay_mul, flags};
    else
        return {lr, weight_decay, 1.f, 0u};
}

// parameter groups: the mask byte names the group (include/dyk_hip.h).  The table arrives as a kernel argument; every workgroup
// turns it into one 16-byte record per group in LDS (slot 0 = frozen) that a lane reads with the byte of its vector -- a wave
// spans 256 elements, i.e. up to four groups.
template <Rule R>
__device__ __forceinline__ const GroupRec* group_table(const DykOptimGroups& gr, float bc1) {
    __shared__ GroupRec tab[DYK_OPT_MAX_GROUPS + 1];
    if (threadIdx.x <= DYK_OPT_MAX_GROUPS) {
        GroupRec r = {0.f, 0.f, 1.f, 0u};
        if (threadIdx.x >= 1 && (int)threadIdx.x <= gr.count) {
            const DykOptimGroup g = gr.g[threadIdx.x - 1];
            r = group_rec<R>(g.lr, g.weight_decay, g.decay_mul, g.flags, bc1);
        }
        tab[threadIdx.x] = r;
    }
    __syncthreads();
    return tab;
}

// the mask word of vector i (entries are 64-element aligned, so the four bytes agree)
__device__ __forceinline__ uint32_t mask_word(const DykOptimDesc& d, long i) { return ((const uint32_t*)d.mask)[i]; }

// rec == NULL: bc1 / bc2_sqrt / first_step as the host formed them from d.step.  Else the record decides: a skipped step only
// clears the gradient (when asked), an applied one takes grad_scale * coef, the bias corrections and SGD's first-step rule
// (the first APPLIED step) from it.  kRec = false: the host knows that rec == NULL -- the plain entries; their launch is 3 us
// (0.4 %) slower on the 116 M-element store when the kernel carries the record's code (profiles/optim_unify.json).
template <Rule R, typename Table, bool kRec>
__global__ __launch_bounds__(256) void step_kernel(DykOptimDesc d, Table gr, const DykGradGuardRec* __restrict__ rec, float bc1,
                                                   float bc2_sqrt, int first_step) {
    constexpr bool kGrouped = !std::is_same<Table, NoGroups>::value;
    const long n4 = d.n >> 2, first = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    float gs = d.grad_scale;
    if (kRec && rec) {
        if (rec->skip) {
            for (long i = first; i < n4; i += stride) clear_grad_vec(d, i);
            return;
        }
        bc1 = rec->bc1;
        bc2_sqrt = rec->bc2_sqrt;
        first_step = rec->applied == 1 ? 1 : 0;
        gs = __fmul_rn(d.grad_scale, rec->coef);
    }
    const GroupRec whole = group_rec<R>(d.lr, d.weight_decay, 1.f, 0u, bc1);   // ungrouped: the record of every live element
    const GroupRec* tab = nullptr;
    uint32_t count = 0;
    if constexpr (kGrouped) {
        tab = group_table<R>(gr, bc1);
        count = (uint32_t)gr.count;
    }
    for (long i = first; i < n4; i += stride) {
        GroupRec r = whole;
        bool frozen;
        if constexpr (kGrouped) {
            const uint32_t k = mask_word(d, i) & 0xffu;
            frozen = k == 0 || k > count;
            if (!frozen) r = tab[k];
        } else {
            frozen = d.mask && mask_word(d, i) == 0;
        }
        if (frozen) {
            clear_grad_vec(d, i);
            continue;
        }
        if constexpr (R == Rule::Adam)
            adam_vec(d, i, gs, r.wd, d.beta1, d.beta2, d.eps, bc2_sqrt, r.a, (r.flags & DYK_OPT_GROUP_DECOUPLED) != 0, r.decay_mul);
        else
            sgd_vec(d, i, gs, r.wd, d.beta1, r.a, first_step);
    }
}

// ---- host side: every check of every entry, the grid and the launch
int check(const DykOptimDesc* d, bool need_v) {
    if (!d || !d->p || !d->g || !d->m || (need_v && !d->v) || d->n <= 0 || (d->n & 3)) return DYK_ERR_ARG;
    if (((uintptr_t)d->p | (uintptr_t)d->g | (uintptr_t)d->m | (uintptr_t)d->v) & 15) return DYK_ERR_ARG;
    if (d->wc && ((uintptr_t)d->wc & 7)) return DYK_ERR_ARG;
    if (d->mask && ((uintptr_t)d->mask & 3)) return DYK_ERR_ARG;
    return DYK_OK;
}

// the checks of the grouped entries that go beyond check(): DYK_OK, DYK_ERR_ARG, or DYK_ERR_UNSUPPORTED for a decoupled group
// where `allow_decoupled` is false (a bad argument anywhere wins over that)
int check_groups(const DykOptimDesc* d, const DykOptimGroups* gr, bool allow_decoupled) {
    if (!d->mask) return DYK_ERR_ARG;
    if (gr->count < 1 || gr->count > DYK_OPT_MAX_GROUPS) return DYK_ERR_ARG;
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

template <Rule R>
void launch_kernel(const DykOptimDesc* d, const DykOptimGroups* gr, const DykGradGuardRec* rec, float bc1, float bc2_sqrt,
                   int first_step, hipStream_t stream) {
    const dim3 grid((int)step_grid(d->n)), block(256);
    if (gr)
        hipLaunchKernelGGL((step_kernel<R, DykOptimGroups, true>), grid, block, 0, stream, *d, *gr, rec, bc1, bc2_sqrt, first_step);
    else if (rec)
        hipLaunchKernelGGL((step_kernel<R, NoGroups, true>), grid, block, 0, stream, *d, NoGroups{}, rec, bc1, bc2_sqrt, first_step);
    else
        hipLaunchKernelGGL((step_kernel<R, NoGroups, false>), grid, block, 0, stream, *d, NoGroups{}, rec, bc1, bc2_sqrt, first_step);
}

// gr == NULL: no parameter groups; rec == NULL: no record, d->step (>= 1) counts the steps
int launch_step(Rule rule, const DykOptimDesc* d, const DykOptimGroups* gr, const DykGradGuardRec* rec, void* stream) {
    const bool adam = rule == Rule::Adam;
    int rc = check(d, adam);
    if (rc) return rc;
    if (rec ? ((uintptr_t)rec & 7) != 0 : d->step <= 0) return DYK_ERR_ARG;
    if (gr && (rc = check_groups(d, gr, adam)) != DYK_OK) return rc;
    float bc1 = 0.f, bc2_sqrt = 0.f;                              // (read from the record when there is one)
    if (adam && !rec) {
        bc1 = (float)(1.0 - pow((double)d->beta1, (double)d->step));
        bc2_sqrt = (float)sqrt(1.0 - pow((double)d->beta2, (double)d->step));
    }
    const int first_step = (!rec && d->step == 1) ? 1 : 0;
    if (adam)
        launch_kernel<Rule::Adam>(d, gr, rec, bc1, bc2_sqrt, first_step, (hipStream_t)stream);
    else
        launch_kernel<Rule::Sgd>(d, gr, rec, bc1, bc2_sqrt, first_step, (hipStream_t)stream);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

}  // namespace

extern "C" int dyk_adam_step(const DykOptimDesc* d, void* stream) { return launch_step(Rule::Adam, d, nullptr, nullptr, stream); }

extern "C" int dyk_sgd_step(const DykOptimDesc* d, void* stream) { return launch_step(Rule::Sgd, d, nullptr, nullptr, stream); }

extern "C" int dyk_adam_step_guarded(const DykOptimDesc* d, const DykGradGuardRec* rec, void* stream) {
    return rec ? launch_step(Rule::Adam, d, nullptr, rec, stream) : DYK_ERR_ARG;
}

extern "C" int dyk_sgd_step_guarded(const DykOptimDesc* d, const DykGradGuardRec* rec, void* stream) {
    return rec ? launch_step(Rule::Sgd, d, nullptr, rec, stream) : DYK_ERR_ARG;
}

extern "C" int dyk_adam_step_groups(const DykOptimDesc* d, const DykOptimGroups* gr, const DykGradGuardRec* rec, void* stream) {
    return gr ? launch_step(Rule::Adam, d, gr, rec, stream) : DYK_ERR_ARG;
}

extern "C" int dyk_sgd_step_groups(const DykOptimDesc* d, const DykOptimGroups* gr, const DykGradGuardRec* rec, void* stream) {
    return gr ? launch_step(Rule::Sgd, d, gr, rec, stream) : DYK_ERR_ARG;
}
