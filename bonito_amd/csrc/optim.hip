// The optimizer step that follows backward(): unscale, global gradient norm, overflow check, clip, AdamW update and the loss-scale
// rule of torch's GradScaler, all on the device and without a host synchronisation (include/bonito_hip.h: bh_optim_norm).
//
// Three kinds of launch on the caller's stream:
//   optim_sumsq_kernel     one workgroup per chunk of OPTIM_CHUNK elements writes the fp32 sum of g^2 of its chunk to its own slot
//   optim_finalise_kernel  one wave adds the slots in fp64 and advances the control block (step, beta products, clip, loss scale)
//   optim_adamw_kernel     the elementwise update, operation by operation in fp32 (this file is built with -ffp-contract=off)
// The table of tensors travels by value in the kernel arguments, at most OPTIM_TENSORS per launch: p.grad is a new allocation after
// every backward(), so a table in device memory would cost a host-to-device copy per step.
#include "bonito_hip.h"
#include "common.h"

#include <math.h>

namespace {

constexpr int OPTIM_TENSORS = 32;                 // tensors per launch
constexpr int OPTIM_THREADS = 256;
constexpr int OPTIM_CHUNK = BH_OPTIM_CHUNK;       // elements per workgroup: 8 float4 per thread
constexpr int OPTIM_VECS = OPTIM_CHUNK / (4 * OPTIM_THREADS);
constexpr long OPTIM_MAX_N = 1L << 40;            // elements per tensor; keeps every chunk count an int

static_assert(OPTIM_CHUNK % (4 * OPTIM_THREADS) == 0, "a chunk is whole float4 rounds of the workgroup");

// first[i] = chunks of this launch in front of tensor i; first[count] = the launch's grid
struct NormTable {
    const float* g[OPTIM_TENSORS];
    long n[OPTIM_TENSORS];
    int first[OPTIM_TENSORS + 1];
};

struct UpdateTable {
    float* p[OPTIM_TENSORS];
    const float* g[OPTIM_TENSORS];
    float* m[OPTIM_TENSORS];
    float* v[OPTIM_TENSORS];
    long n[OPTIM_TENSORS];
    int first[OPTIM_TENSORS + 1];
    unsigned aligned16;                           // bit i: p, g, m and v of tensor i are all 16-byte aligned
};

thread_local int g_last_kernel = 0;

inline long chunks_of(long n) { return (n + OPTIM_CHUNK - 1) / OPTIM_CHUNK; }

// The thread-to-element assignment is the same on the vector and the scalar path: thread t takes elements 4 (t + 256 k) .. + 3 of
// the chunk for k = 0 .. OPTIM_VECS - 1 and adds their squares in that order, so the sums depend on the sizes alone.
__global__ __launch_bounds__(OPTIM_THREADS) void optim_sumsq_kernel(NormTable tab, int count, float* __restrict__ slots) {
    const int b = blockIdx.x;
    int t = 0;
    while (t + 1 < count && tab.first[t + 1] <= b) ++t;
    const long base = (long)(b - tab.first[t]) * OPTIM_CHUNK;
    const long left = tab.n[t] - base;
    const int cnt = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;
    const float* g = tab.g[t] + base;
    const bool vec = ((uintptr_t)g & 15) == 0;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < OPTIM_VECS; ++k) {
        const int i = 4 * ((int)threadIdx.x + OPTIM_THREADS * k);
        if (i + 4 <= cnt) {
            float x0, x1, x2, x3;
            if (vec) {
                const float4 x = *reinterpret_cast<const float4*>(g + i);
                x0 = x.x; x1 = x.y; x2 = x.z; x3 = x.w;
            } else {
                x0 = g[i]; x1 = g[i + 1]; x2 = g[i + 2]; x3 = g[i + 3];
            }
            acc += x0 * x0;
            acc += x1 * x1;
            acc += x2 * x2;
            acc += x3 * x3;
        } else {
            for (int j = i; j < cnt; ++j) acc += g[j] * g[j];
        }
    }
    // a fixed tree inside the wave, then the four waves in order
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    __shared__ float wave_sum[OPTIM_THREADS / 64];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = wave_sum[0];
        for (int w = 1; w < OPTIM_THREADS / 64; ++w) s += wave_sum[w];
        slots[b] = s;
    }
}

// One wave. Lane l adds slots l, l + 64, ... in fp64, lane 0 then adds the 64 lane sums in lane order: a fixed order for a given
// number of slots. fp64 holds a sum of up to 2^29 fp32 values of equal size exactly, so the order shows in no test.
__global__ __launch_bounds__(64) void optim_finalise_kernel(const float* __restrict__ slots, long n_slots, double* __restrict__ ctl,
                                                            double max_norm, int use_scale, double growth, double backoff,
                                                            int growth_interval, double beta1, double beta2) {
    __shared__ double lane_sum[64];
    double s = 0.0;
    for (long i = threadIdx.x; i < n_slots; i += 64) s += (double)slots[i];
    lane_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int l = 0; l < 64; ++l) sum += lane_sum[l];

    const double scale = use_scale ? ctl[BH_OPTIM_SCALE] : 1.0;
    const bool skipped = !isfinite(sum);
    const double norm = sqrt(sum) / scale;
    ctl[BH_OPTIM_GRAD_NORM] = norm;
    ctl[BH_OPTIM_SKIPPED] = skipped ? 1.0 : 0.0;
    ctl[BH_OPTIM_SCALE_USED] = scale;
    if (!skipped) {
        const double b1p = ctl[BH_OPTIM_BETA1_POW] * beta1, b2p = ctl[BH_OPTIM_BETA2_POW] * beta2;
        const double clip = max_norm > 0.0 ? fmin(1.0, max_norm / (norm + 1e-6)) : 1.0;
        ctl[BH_OPTIM_STEP] += 1.0;
        ctl[BH_OPTIM_BETA1_POW] = b1p;
        ctl[BH_OPTIM_BETA2_POW] = b2p;
        ctl[BH_OPTIM_CLIP_COEF] = clip;
        ctl[BH_OPTIM_GRAD_MUL] = clip / scale;
        ctl[BH_OPTIM_BIAS1] = 1.0 - b1p;
        ctl[BH_OPTIM_BIAS2_SQRT] = sqrt(1.0 - b2p);
    } else {
        ctl[BH_OPTIM_CLIP_COEF] = 0.0;
        ctl[BH_OPTIM_GRAD_MUL] = 0.0;
    }
    if (use_scale) {                              // torch.amp.GradScaler.update
        if (skipped) {
            ctl[BH_OPTIM_SCALE] = scale * backoff;
            ctl[BH_OPTIM_GROWTH_TRACKER] = 0.0;
        } else {
            const double tracker = ctl[BH_OPTIM_GROWTH_TRACKER] + 1.0;
            if (tracker == (double)growth_interval) {
                ctl[BH_OPTIM_SCALE] = scale * growth;
                ctl[BH_OPTIM_GROWTH_TRACKER] = 0.0;
            } else {
                ctl[BH_OPTIM_GROWTH_TRACKER] = tracker;
            }
        }
    }
}

struct AdamScalars {
    float grad_mul, decay, b1, one_minus_b1, b2, one_minus_b2, bias2_sqrt, eps, step_size;
};

// torch's AdamW, decoupled decay first; every operation rounds to fp32 (no contraction in this file)
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const AdamScalars& s) {
    const float gs = g * s.grad_mul;
    p = p * s.decay;
    m = s.b1 * m + s.one_minus_b1 * gs;
    v = s.b2 * v + (s.one_minus_b2 * gs) * gs;
    const float denom = sqrtf(v) / s.bias2_sqrt + s.eps;
    p = p - s.step_size * (m / denom);
}

__global__ __launch_bounds__(OPTIM_THREADS) void optim_adamw_kernel(UpdateTable tab, int count, const double* __restrict__ ctl, double lr,
                                                                   float decay, float b1, float one_minus_b1, float b2,
                                                                   float one_minus_b2, float eps) {
    if (ctl[BH_OPTIM_SKIPPED] != 0.0) return;     // an overflowed step: no byte of p, m, v changes
    AdamScalars s;
    s.grad_mul = (float)ctl[BH_OPTIM_GRAD_MUL];
    s.decay = decay;
    s.b1 = b1;
    s.one_minus_b1 = one_minus_b1;
    s.b2 = b2;
    s.one_minus_b2 = one_minus_b2;
    s.bias2_sqrt = (float)ctl[BH_OPTIM_BIAS2_SQRT];
    s.eps = eps;
    s.step_size = (float)(lr / ctl[BH_OPTIM_BIAS1]);

    const int b = blockIdx.x;
    int t = 0;
    while (t + 1 < count && tab.first[t + 1] <= b) ++t;
    const long base = (long)(b - tab.first[t]) * OPTIM_CHUNK;
    const long left = tab.n[t] - base;
    const int cnt = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;
    float* p = tab.p[t] + base;
    const float* g = tab.g[t] + base;
    float* m = tab.m[t] + base;
    float* v = tab.v[t] + base;
    const bool vec = (tab.aligned16 >> t) & 1u;   // the chunk offset is a multiple of 16 bytes
#pragma unroll 2
    for (int k = 0; k < OPTIM_VECS; ++k) {
        const int i = 4 * ((int)threadIdx.x + OPTIM_THREADS * k);
        if (vec && i + 4 <= cnt) {
            float4 pp = *reinterpret_cast<const float4*>(p + i);
            const float4 gg = *reinterpret_cast<const float4*>(g + i);
            float4 mm = *reinterpret_cast<const float4*>(m + i);
            float4 vv = *reinterpret_cast<const float4*>(v + i);
            adamw_element(pp.x, gg.x, mm.x, vv.x, s);
            adamw_element(pp.y, gg.y, mm.y, vv.y, s);
            adamw_element(pp.z, gg.z, mm.z, vv.z, s);
            adamw_element(pp.w, gg.w, mm.w, vv.w, s);
            *reinterpret_cast<float4*>(p + i) = pp;
            *reinterpret_cast<float4*>(m + i) = mm;
            *reinterpret_cast<float4*>(v + i) = vv;
        } else {
            const int end = i + 4 < cnt ? i + 4 : cnt;
            for (int j = i; j < end; ++j) {
                float pj = p[j], mj = m[j], vj = v[j];
                adamw_element(pj, g[j], mj, vj, s);
                p[j] = pj;
                m[j] = mj;
                v[j] = vj;
            }
        }
    }
}

int check_sizes(const char* what, const long* n, int n_tensors) {
    BH_REQUIRE(n != nullptr && n_tensors >= 1, "%s: bad arguments (null size table or n_tensors = %d < 1)", what, n_tensors);
    for (int i = 0; i < n_tensors; ++i)
        BH_REQUIRE(n[i] >= 1 && n[i] <= OPTIM_MAX_N, "%s: tensor %d has n = %ld elements (1 .. 2^40 are served)", what, i, n[i]);
    return 0;
}

int check_betas(const char* what, double beta1, double beta2) {
    BH_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas (%g, %g) must lie in [0, 1)", what, beta1, beta2);
    return 0;
}

// the chunk prefix of tensors [lo, hi) of a launch; -2 when the grid would pass 2^31 - 1 workgroups
template <class Table>
int fill_first(const char* what, Table& tab, const long* n, int lo, int hi) {
    long total = 0;
    for (int i = lo; i < hi; ++i) {
        tab.n[i - lo] = n[i];
        tab.first[i - lo] = (int)total;
        total += chunks_of(n[i]);
        BH_REQUIRE(total < (1L << 31), "%s: tensors %d .. %d need %ld workgroups in one launch (at most 2^31 - 1)", what, lo, i, total);
    }
    tab.first[hi - lo] = (int)total;
    return 0;
}

}  // namespace

extern "C" {

int bh_optim_last_kernel(void) { return g_last_kernel; }

int bh_optim_chunk(void) { return OPTIM_CHUNK; }

size_t bh_optim_workspace(const long* n, int n_tensors) {
    if (check_sizes("bh_optim_workspace", n, n_tensors) != 0) return 0;
    long slots = 0;
    for (int i = 0; i < n_tensors; ++i) slots += chunks_of(n[i]);
    return (size_t)slots * sizeof(float);
}

int bh_optim_norm(const float* const* g, const long* n, int n_tensors, double* ctl, double max_norm, int use_scale, double growth,
                  double backoff, int growth_interval, double beta1, double beta2, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "bh_optim_norm";
    BH_REQUIRE(g != nullptr && ctl != nullptr && workspace != nullptr, "%s: bad arguments (null pointer)", what);
    if (int rc = check_sizes(what, n, n_tensors)) return rc;
    for (int i = 0; i < n_tensors; ++i)
        BH_REQUIRE(g[i] != nullptr && ((uintptr_t)g[i] & 3) == 0, "%s: gradient %d is null or not 4-byte aligned", what, i);
    if (int rc = check_betas(what, beta1, beta2)) return rc;
    BH_REQUIRE(!(max_norm != max_norm), "%s: max_norm is NaN", what);
    if (use_scale)
        BH_REQUIRE(growth >= 1.0 && backoff > 0.0 && backoff <= 1.0 && growth_interval >= 1 && isfinite(growth),
                   "%s: loss scale rule growth=%g backoff=%g growth_interval=%d (growth >= 1, 0 < backoff <= 1, interval >= 1)", what, growth,
                   backoff, growth_interval);
    const size_t need = bh_optim_workspace(n, n_tensors);
    BH_REQUIRE(((uintptr_t)workspace & 3) == 0 && workspace_bytes >= need, "%s: workspace of %zu bytes is too small or misaligned (%zu needed)",
               what, workspace_bytes, need);
    BH_REQUIRE(((uintptr_t)ctl & 7) == 0, "%s: the control block must be 8-byte aligned", what);
    // every launch's table is checked before the first launch
    for (int lo = 0; lo < n_tensors; lo += OPTIM_TENSORS) {
        NormTable tab = {};
        if (int rc = fill_first(what, tab, n, lo, lo + OPTIM_TENSORS < n_tensors ? lo + OPTIM_TENSORS : n_tensors)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    float* slots = (float*)workspace;
    long slot0 = 0;
    for (int lo = 0; lo < n_tensors; lo += OPTIM_TENSORS) {
        const int hi = lo + OPTIM_TENSORS < n_tensors ? lo + OPTIM_TENSORS : n_tensors;
        NormTable tab = {};
        fill_first(what, tab, n, lo, hi);
        for (int i = lo; i < hi; ++i) tab.g[i - lo] = g[i];
        const int grid = tab.first[hi - lo];
        hipLaunchKernelGGL(optim_sumsq_kernel, dim3(grid), dim3(OPTIM_THREADS), 0, st, tab, hi - lo, slots + slot0);
        BH_CHECK_HIP(hipGetLastError());
        slot0 += grid;
    }
    hipLaunchKernelGGL(optim_finalise_kernel, dim3(1), dim3(64), 0, st, slots, slot0, ctl, max_norm, use_scale, growth, backoff,
                       growth_interval, beta1, beta2);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

int bh_optim_update(float* const* p, const float* const* g, float* const* m, float* const* v, const long* n, int n_tensors,
                    const double* ctl, double lr, double beta1, double beta2, double eps, double weight_decay, void* stream) {
    const char* what = "bh_optim_update";
    BH_REQUIRE(p != nullptr && g != nullptr && m != nullptr && v != nullptr && ctl != nullptr, "%s: bad arguments (null pointer)", what);
    if (int rc = check_sizes(what, n, n_tensors)) return rc;
    for (int i = 0; i < n_tensors; ++i)
        BH_REQUIRE(p[i] != nullptr && g[i] != nullptr && m[i] != nullptr && v[i] != nullptr
                       && (((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i]) & 3) == 0,
                   "%s: tensor %d has a null or not 4-byte aligned pointer", what, i);
    if (int rc = check_betas(what, beta1, beta2)) return rc;
    BH_REQUIRE(lr >= 0.0 && isfinite(lr), "%s: lr = %g must be finite and not negative", what, lr);
    BH_REQUIRE(eps >= 0.0 && isfinite(eps), "%s: eps = %g must be finite and not negative", what, eps);
    BH_REQUIRE(weight_decay >= 0.0 && isfinite(weight_decay), "%s: weight_decay = %g must be finite and not negative", what, weight_decay);
    BH_REQUIRE(((uintptr_t)ctl & 7) == 0, "%s: the control block must be 8-byte aligned", what);
    for (int lo = 0; lo < n_tensors; lo += OPTIM_TENSORS) {
        UpdateTable tab = {};
        if (int rc = fill_first(what, tab, n, lo, lo + OPTIM_TENSORS < n_tensors ? lo + OPTIM_TENSORS : n_tensors)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    int paths = 0;
    for (int lo = 0; lo < n_tensors; lo += OPTIM_TENSORS) {
        const int hi = lo + OPTIM_TENSORS < n_tensors ? lo + OPTIM_TENSORS : n_tensors;
        UpdateTable tab = {};
        fill_first(what, tab, n, lo, hi);
        for (int i = lo; i < hi; ++i) {
            tab.p[i - lo] = p[i];
            tab.g[i - lo] = g[i];
            tab.m[i - lo] = m[i];
            tab.v[i - lo] = v[i];
            const bool a16 = (((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i]) & 15) == 0;
            if (a16) tab.aligned16 |= 1u << (i - lo);
            paths |= a16 ? BH_OPTIM_K_VECTOR : BH_OPTIM_K_SCALAR;
        }
        hipLaunchKernelGGL(optim_adamw_kernel, dim3(tab.first[hi - lo]), dim3(OPTIM_THREADS), 0, st, tab, hi - lo, ctl, lr,
                           (float)(1.0 - lr * weight_decay), (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                           (float)eps);
        BH_CHECK_HIP(hipGetLastError());
    }
    g_last_kernel = paths;
    return 0;
}

}  // extern "C"
