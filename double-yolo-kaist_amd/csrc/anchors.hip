// Anchor clustering on the device (dyk_anchor_assign, dyk_anchor_median, dyk_anchor_fitness; the rule is in include/dyk_hip.h):
// the IoU k-means assignment, the exact per-coordinate median of every cluster and the fitness of G anchor candidates at once.
// Every floating-point operation is rounded on its own (the pragma below turns contraction off for this file; the Makefile's
// default is -ffp-contract=on), divisions are IEEE divisions, and whatever is summed in floating point is summed in the order the
// header states.  Counts go through INTEGER atomics only, so every output is a pure function of the inputs.
#include <float.h>
#include "dyk_common.h"
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / DYK_WAVE;
constexpr int kMaxK = DYK_ANCHOR_MAX_K;
constexpr int kFitItem = DYK_ANCHOR_FIT_ITEM;
constexpr int kFitPer = kFitItem / kBlock;               // boxes per thread of a fitness item: 4
static_assert(kFitPer * kBlock == kFitItem, "a fitness item is a whole number of boxes per thread");
static_assert(sizeof(DykAnchorAssignDesc) == 48 && sizeof(DykAnchorMedianDesc) == 56 && sizeof(DykAnchorFitnessDesc) == 88, "ABI layout");

template <typename T> struct Bits;
template <> struct Bits<float> {
    typedef uint32_t type;
    static __device__ inline bool good(float v) { return v > 0.f && v <= FLT_MAX; }
};
template <> struct Bits<double> {
    typedef unsigned long long type;
    static __device__ inline bool good(double v) { return v > 0.0 && v <= DBL_MAX; }
};

// ------------------------------------------------------------------------------------------------ assignment
template <typename T>
__global__ __launch_bounds__(kBlock) void anchor_assign_kernel(const T* __restrict__ wh, const T* __restrict__ c, int32_t* __restrict__ nearest,
                                                               int32_t* __restrict__ stats, int N, int K) {
    __shared__ T s_c[kMaxK][2];
    __shared__ T s_area[kMaxK];
    __shared__ int s_cnt[kMaxK + 2];
    const int t = threadIdx.x;
    if (t < K) {
        const T cw = c[2 * t], ch = c[2 * t + 1];
        s_c[t][0] = cw;
        s_c[t][1] = ch;
        s_area[t] = cw * ch;
    }
    if (t < kMaxK + 2) s_cnt[t] = 0;
    __syncthreads();
    const long i = (long)blockIdx.x * kBlock + t;
    if (i < N) {
        const T w = wh[2 * i], h = wh[2 * i + 1];
        const bool ok = Bits<T>::good(w) && Bits<T>::good(h);
        const T area = w * h;
        int best = 0;
        T dbest = (T)0;
        for (int k = 0; k < K; ++k) {
            const T cw = s_c[k][0], ch = s_c[k][1];
            const T inter = (w < cw ? w : cw) * (h < ch ? h : ch);
            const T iou = inter / ((area + s_area[k]) - inter);
            const T d = (T)1 - iou;
            if (k == 0 || d < dbest) {                   // strict: the first minimum stays
                dbest = d;
                best = k;
            }
        }
        if (!ok) best = 0;
        const int before = nearest[i];
        nearest[i] = best;
        atomicAdd(&s_cnt[best], 1);
        if (before != best) atomicAdd(&s_cnt[kMaxK], 1);
        if (!ok) atomicAdd(&s_cnt[kMaxK + 1], 1);
    }
    __syncthreads();
    if (t < K && s_cnt[t]) atomicAdd(&stats[t], s_cnt[t]);
    if (t >= kMaxK && t < kMaxK + 2 && s_cnt[t]) atomicAdd(&stats[K + (t - kMaxK)], s_cnt[t]);
}

// ------------------------------------------------------------------------------------------------ median
// Radix select of the lower middle of all 2K (cluster, coordinate) selections at once, 8 bits per pass from the top.  Per pass
// two launches: every workgroup histograms its share of the boxes in LDS (256 bins per selection, 16 clusters per launch, so
// 32 KB) and adds the non-zero bins to the workspace with integer atomics; then one workgroup per selection picks the digit.
// The kernel boundary orders the two; nothing is handed over inside a launch.
struct SelState {
    unsigned long long prefix;     // the digits found so far, in place
    unsigned long long minkey;     // the smallest member above the lower middle (the last launches)
    unsigned rank;                 // rank of the lower middle among the members that share the prefix
    unsigned m;                    // members of the cluster
    unsigned below;                // members below the prefix
    unsigned equal;                // members in the chosen bin (after the last pass: equal to the lower middle)
};
static_assert(sizeof(SelState) == 32, "workspace layout");
constexpr int kSelClusters = 16;                         // clusters per histogram launch
constexpr int kSelMaxBlocks = 1024;

__device__ inline bool sel_needs_upper(const SelState& st) { return st.m && !(st.m & 1u) && st.m / 2 >= st.below + st.equal; }

template <typename T>
__global__ __launch_bounds__(kBlock) void anchor_median_hist_kernel(const T* __restrict__ wh, const int32_t* __restrict__ nearest,
                                                                    const SelState* __restrict__ state, unsigned* __restrict__ ghist, int N, int K,
                                                                    int kbase, int p) {
    typedef typename Bits<T>::type U;
    constexpr int kPasses = (int)sizeof(U);
    __shared__ unsigned s_h[2 * kSelClusters * 256];
    __shared__ U s_prefix[2 * kSelClusters];
    const int t = threadIdx.x;
    const int kn = K - kbase < kSelClusters ? K - kbase : kSelClusters;      // clusters of this launch
    const int shift = 8 * (kPasses - 1 - p);
    for (int i = t; i < 2 * kn * 256; i += kBlock) s_h[i] = 0;
    if (t < 2 * kn) s_prefix[t] = (U)state[2 * kbase + t].prefix;
    __syncthreads();
    const U* keys = (const U*)wh;
    for (long i = (long)blockIdx.x * kBlock + t; i < N; i += (long)gridDim.x * kBlock) {
        const unsigned k = (unsigned)(nearest[i] - kbase);
        if (k >= (unsigned)kn) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const U key = keys[2 * i + j];
            const int sel = 2 * (int)k + j;
            // the bits above this pass's digit equal the prefix found so far (pass 0: nothing above)
            if (p == 0 || ((key ^ s_prefix[sel]) >> (shift + 8)) == 0) atomicAdd(&s_h[sel * 256 + ((unsigned)(key >> shift) & 255u)], 1u);
        }
    }
    __syncthreads();
    for (int i = t; i < 2 * kn * 256; i += kBlock)
        if (s_h[i]) atomicAdd(&ghist[2 * kbase * 256 + i], s_h[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void anchor_median_pick_kernel(SelState* __restrict__ state, unsigned* __restrict__ ghist, int p) {
    typedef typename Bits<T>::type U;
    constexpr int kPasses = (int)sizeof(U);
    __shared__ unsigned s_b[256];
    const int sel = blockIdx.x, t = threadIdx.x;
    s_b[t] = ghist[sel * 256 + t];
    ghist[sel * 256 + t] = 0;                             // ready for the next pass
    __syncthreads();
    if (t != 0) return;
    SelState st = state[sel];
    if (p == 0) {
        unsigned m = 0;
        for (int b = 0; b < 256; ++b) m += s_b[b];
        st.m = m;
        st.below = 0;
        st.rank = m ? (m - 1) / 2 : 0;
        st.prefix = 0;
    }
    if (st.m) {
        unsigned cum = 0;
        int b = 0;
        while (b < 255 && cum + s_b[b] <= st.rank) cum += s_b[b++];
        st.rank -= cum;
        st.below += cum;
        st.equal = s_b[b];
        st.prefix |= (unsigned long long)b << (8 * (kPasses - 1 - p));
    }
    st.minkey = ~0ull;
    state[sel] = st;
}

// even counts whose upper middle is not the lower middle's value: it is the smallest member above it
template <typename T>
__global__ __launch_bounds__(kBlock) void anchor_median_upper_kernel(const T* __restrict__ wh, const int32_t* __restrict__ nearest, SelState* __restrict__ state,
                                                                     int N, int K) {
    typedef typename Bits<T>::type U;
    __shared__ unsigned long long s_min[2 * kMaxK];
    __shared__ U s_lo[2 * kMaxK];
    __shared__ int s_need[2 * kMaxK];
    const int t = threadIdx.x;
    int need = 0;
    if (t < 2 * K) {
        const SelState st = state[t];
        need = sel_needs_upper(st) ? 1 : 0;
        s_need[t] = need;
        s_lo[t] = (U)st.prefix;
        s_min[t] = ~0ull;
    }
    if (!__syncthreads_or(need)) return;
    const U* keys = (const U*)wh;
    for (long i = (long)blockIdx.x * kBlock + t; i < N; i += (long)gridDim.x * kBlock) {
        const unsigned k = (unsigned)nearest[i];
        if (k >= (unsigned)K) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int sel = 2 * (int)k + j;
            if (!s_need[sel]) continue;
            const U key = keys[2 * i + j];
            if (key > s_lo[sel] && (unsigned long long)key < s_min[sel]) atomicMin(&s_min[sel], (unsigned long long)key);
        }
    }
    __syncthreads();
    if (t < 2 * K && s_need[t] && s_min[t] != ~0ull) atomicMin(&state[t].minkey, s_min[t]);
}

template <typename T>
__global__ __launch_bounds__(DYK_WAVE) void anchor_median_write_kernel(const SelState* __restrict__ state, T* __restrict__ c, int K) {
    typedef typename Bits<T>::type U;
    const int t = threadIdx.x;
    if (t >= 2 * K) return;
    const SelState st = state[t];
    if (st.m == 0) return;                                // an empty cluster keeps its centre
    const T a = __builtin_bit_cast(T, (U)st.prefix);
    const T b = sel_needs_upper(st) ? __builtin_bit_cast(T, (U)st.minkey) : a;
    c[t] = (st.m & 1u) ? a : (a + b) / (T)2;
}

template <typename T>
int launch_median(const DykAnchorMedianDesc* d, hipStream_t s) {
    constexpr int kPasses = (int)sizeof(typename Bits<T>::type);
    SelState* state = (SelState*)d->ws;
    unsigned* ghist = (unsigned*)(state + 2 * d->K);
    const int blocks = dyk_div_up(d->N, kBlock * 4) < kSelMaxBlocks ? dyk_div_up(d->N, kBlock * 4) : kSelMaxBlocks;
    for (int p = 0; p < kPasses; ++p) {
        for (int kbase = 0; kbase < d->K; kbase += kSelClusters) {
            hipLaunchKernelGGL(anchor_median_hist_kernel<T>, dim3(blocks), dim3(kBlock), 0, s, (const T*)d->wh, d->nearest, (const SelState*)state, ghist,
                               d->N, d->K, kbase, p);
            DYK_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(anchor_median_pick_kernel<T>, dim3(2 * d->K), dim3(256), 0, s, state, ghist, p);
        DYK_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(anchor_median_upper_kernel<T>, dim3(blocks), dim3(kBlock), 0, s, (const T*)d->wh, d->nearest, state, d->N, d->K);
    DYK_LAUNCH_CHECK();
    hipLaunchKernelGGL(anchor_median_write_kernel<T>, dim3(1), dim3(DYK_WAVE), 0, s, (const SelState*)state, (T*)d->c, d->K);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

// ------------------------------------------------------------------------------------------------ fitness
// workspace: double sum[G][nitems], double tmax[G][nitems][K], int32 hit[G][nitems]
template <typename T>
__global__ __launch_bounds__(kBlock) void anchor_fitness_partials_kernel(const T* __restrict__ wh, const double* __restrict__ a, double thr, int N, int K,
                                                                         int nitems, double* __restrict__ ws_sum, double* __restrict__ ws_tmax,
                                                                         int32_t* __restrict__ ws_hit) {
    __shared__ double s_a[kMaxK][2];
    __shared__ double s_t[kWaves][kMaxK];
    __shared__ double s_sum[kWaves];
    __shared__ int s_hit[kWaves];
    const int item = blockIdx.x, g = blockIdx.y;
    const int t = threadIdx.x, lane = t & (DYK_WAVE - 1), wave = t / DYK_WAVE;
    if (t < 2 * K) s_a[t >> 1][t & 1] = a[(long)g * 2 * K + t];
    __syncthreads();
    double w[kFitPer], h[kFitPer], b[kFitPer];
    bool in[kFitPer];
#pragma unroll
    for (int u = 0; u < kFitPer; ++u) {
        const long i = (long)item * kFitItem + t + u * kBlock;
        in[u] = i < N;
        w[u] = in[u] ? (double)wh[2 * i] : 1.0;
        h[u] = in[u] ? (double)wh[2 * i + 1] : 1.0;
        b[u] = 0.0;
    }
    for (int k = 0; k < K; ++k) {
        const double aw = s_a[k][0], ah = s_a[k][1];
        double tk = 0.0;                                 // every x is >= 0: 0 is the identity of these maxima
#pragma unroll
        for (int u = 0; u < kFitPer; ++u) {
            const double rw = w[u] / aw, rh = h[u] / ah;
            const double qw = 1.0 / rw, qh = 1.0 / rh;
            const double mw = rw < qw ? rw : qw, mh = rh < qh ? rh : qh;
            double x = mw < mh ? mw : mh;
            x = in[u] ? x : 0.0;
            b[u] = x > b[u] ? x : b[u];
            tk = x > tk ? x : tk;
        }
#pragma unroll
        for (int off = DYK_WAVE / 2; off > 0; off >>= 1) {
            const double o = __shfl_down(tk, off);
            tk = o > tk ? o : tk;
        }
        if (lane == 0) s_t[wave][k] = tk;
    }
    double acc = 0.0;
    int hit = 0;
#pragma unroll
    for (int u = 0; u < kFitPer; ++u) {                  // the thread's boxes in order; an absent box adds +0.0
        const bool over = b[u] > thr;
        acc += over ? b[u] : 0.0;
        hit += over ? 1 : 0;
    }
#pragma unroll
    for (int off = DYK_WAVE / 2; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off);
        hit += __shfl_down(hit, off);
    }
    if (lane == 0) {
        s_sum[wave] = acc;
        s_hit[wave] = hit;
    }
    __syncthreads();
    const long slot = (long)g * nitems + item;
    if (t == 0) {
        ws_sum[slot] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        ws_hit[slot] = s_hit[0] + s_hit[1] + s_hit[2] + s_hit[3];
    }
    if (t < K) {
        double m = s_t[0][t];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) m = s_t[wv][t] > m ? s_t[wv][t] : m;
        ws_tmax[slot * K + t] = m;
    }
}

__global__ __launch_bounds__(kBlock) void anchor_fitness_fold_kernel(const double* __restrict__ ws_sum, const double* __restrict__ ws_tmax,
                                                                     const int32_t* __restrict__ ws_hit, double thr, int N, int K, int G, int nitems,
                                                                     double* __restrict__ fit_boxes, double* __restrict__ fit_anchors,
                                                                     int32_t* __restrict__ hit_boxes, int32_t* __restrict__ hit_anchors) {
    const int g = blockIdx.x * kWaves + threadIdx.x / DYK_WAVE;      // one wave per candidate
    if (g >= G) return;
    const int lane = threadIdx.x & (DYK_WAVE - 1);
    const long base = (long)g * nitems;
    double acc = 0.0;
    int hit = 0;
    for (int p = lane; p < nitems; p += DYK_WAVE) {                  // lane l: items l, l + 64, ... in that order
        acc += ws_sum[base + p];
        hit += ws_hit[base + p];
    }
#pragma unroll
    for (int off = DYK_WAVE / 2; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off);
        hit += __shfl_down(hit, off);
    }
    double fa = 0.0;
    int ha = 0;
    for (int k = 0; k < K; ++k) {
        double m = 0.0;
        for (int p = lane; p < nitems; p += DYK_WAVE) {
            const double v = ws_tmax[(base + p) * K + k];
            m = v > m ? v : m;
        }
#pragma unroll
        for (int off = DYK_WAVE / 2; off > 0; off >>= 1) {
            const double o = __shfl_down(m, off);
            m = o > m ? o : m;
        }
        const bool over = m > thr;                                   // (only lane 0 holds the whole maximum, and only it writes)
        fa += over ? m : 0.0;
        ha += over ? 1 : 0;
    }
    if (lane == 0) {
        fit_boxes[g] = acc / (double)N;
        hit_boxes[g] = hit;
        fit_anchors[g] = fa / (double)K;
        hit_anchors[g] = ha;
    }
}

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
inline bool shape_ok(int N, int K, int eb) { return N >= 1 && N <= DYK_ANCHOR_MAX_N && K >= 1 && K <= kMaxK && (eb == 4 || eb == 8); }

}  // namespace

extern "C" int dyk_anchor_assign(const DykAnchorAssignDesc* d, void* stream) {
    if (!d || !d->wh || !d->c || !d->nearest || !d->stats || !shape_ok(d->N, d->K, d->elem_bytes)) return DYK_ERR_ARG;
    if (misaligned(d->wh, d->elem_bytes) || misaligned(d->c, d->elem_bytes) || misaligned(d->nearest, 4) || misaligned(d->stats, 4)) return DYK_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    DYK_HIP_TRY(hipMemsetAsync(d->stats, 0, sizeof(int32_t) * (d->K + 2), s));
    const dim3 grid(dyk_div_up(d->N, kBlock));
    if (d->elem_bytes == 4)
        hipLaunchKernelGGL(anchor_assign_kernel<float>, grid, dim3(kBlock), 0, s, (const float*)d->wh, (const float*)d->c, d->nearest, d->stats, d->N, d->K);
    else
        hipLaunchKernelGGL(anchor_assign_kernel<double>, grid, dim3(kBlock), 0, s, (const double*)d->wh, (const double*)d->c, d->nearest, d->stats, d->N,
                           d->K);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}

extern "C" int64_t dyk_anchor_median_ws_bytes(int32_t K) {
    if (K < 1 || K > kMaxK) return 0;
    return (int64_t)2 * K * (sizeof(SelState) + 256 * sizeof(unsigned));
}

extern "C" int dyk_anchor_median(const DykAnchorMedianDesc* d, void* stream) {
    if (!d || !d->wh || !d->c || !d->nearest || !d->ws || !shape_ok(d->N, d->K, d->elem_bytes)) return DYK_ERR_ARG;
    if (misaligned(d->wh, d->elem_bytes) || misaligned(d->c, d->elem_bytes) || misaligned(d->nearest, 4) || misaligned(d->ws, 8)) return DYK_ERR_ARG;
    const int64_t need = dyk_anchor_median_ws_bytes(d->K);
    if (d->ws_bytes < need) return DYK_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    DYK_HIP_TRY(hipMemsetAsync(d->ws, 0, (size_t)need, s));
    return d->elem_bytes == 4 ? launch_median<float>(d, s) : launch_median<double>(d, s);
}

extern "C" int64_t dyk_anchor_fitness_ws_bytes(int32_t N, int32_t G, int32_t K) {
    if (!shape_ok(N, K, 8) || G < 1 || G > DYK_ANCHOR_MAX_G) return 0;
    const int64_t slots = (int64_t)G * dyk_div_up(N, kFitItem);
    return ((slots * (8 + 8 * (int64_t)K + 4)) + 7) & ~(int64_t)7;
}

extern "C" int dyk_anchor_fitness(const DykAnchorFitnessDesc* d, void* stream) {
    if (!d || !d->wh || !d->a || !d->ws || !d->fit_boxes || !d->fit_anchors || !d->hit_boxes || !d->hit_anchors) return DYK_ERR_ARG;
    if (!shape_ok(d->N, d->K, d->elem_bytes) || d->G < 1 || d->G > DYK_ANCHOR_MAX_G || !(d->thr >= -DBL_MAX && d->thr <= DBL_MAX)) return DYK_ERR_ARG;
    if (misaligned(d->wh, d->elem_bytes) || misaligned(d->a, 8) || misaligned(d->ws, 8) || misaligned(d->fit_boxes, 8) || misaligned(d->fit_anchors, 8) ||
        misaligned(d->hit_boxes, 4) || misaligned(d->hit_anchors, 4))
        return DYK_ERR_ARG;
    const int64_t need = dyk_anchor_fitness_ws_bytes(d->N, d->G, d->K);
    if (need <= 0 || d->ws_bytes < need) return DYK_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nitems = dyk_div_up(d->N, kFitItem);
    const int64_t slots = (int64_t)d->G * nitems;
    double* ws_sum = (double*)d->ws;
    double* ws_tmax = ws_sum + slots;
    int32_t* ws_hit = (int32_t*)(ws_tmax + slots * d->K);
    const dim3 grid(nitems, d->G);
    if (d->elem_bytes == 4)
        hipLaunchKernelGGL(anchor_fitness_partials_kernel<float>, grid, dim3(kBlock), 0, s, (const float*)d->wh, d->a, d->thr, d->N, d->K, nitems, ws_sum,
                           ws_tmax, ws_hit);
    else
        hipLaunchKernelGGL(anchor_fitness_partials_kernel<double>, grid, dim3(kBlock), 0, s, (const double*)d->wh, d->a, d->thr, d->N, d->K, nitems, ws_sum,
                           ws_tmax, ws_hit);
    DYK_LAUNCH_CHECK();
    hipLaunchKernelGGL(anchor_fitness_fold_kernel, dim3(dyk_div_up(d->G, kWaves)), dim3(kBlock), 0, s, (const double*)ws_sum, (const double*)ws_tmax,
                       (const int32_t*)ws_hit, d->thr, d->N, d->K, d->G, nitems, d->fit_boxes, d->fit_anchors, d->hit_boxes, d->hit_anchors);
    DYK_LAUNCH_CHECK();
    return DYK_OK;
}
