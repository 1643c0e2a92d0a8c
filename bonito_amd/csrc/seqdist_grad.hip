// Gradients of the two CTC-CRF log-sums of csrc/seqdist.hip on gfx950: what makes CTC_CRF.ctc_loss (reference bonito/crf/model.py:126-139)
// a training loss and SequenceDist.posteriors available for either layout. The reference differentiates koi.ctc.logZ_cu / logZ_cu_sparse;
// the gradient of a log-sum over paths is the posterior occupancy of every edge, so both kernels are an alpha-beta pass.
//
// Chain gradient (bh_crf_seq_logz_grad): the chain, layouts, strides, target types and range of bh_crf_seq_logz (seqdist.hip).
//     alpha_t = the Log scan before step t (alpha_0 = [0, -inf, ...]);  beta_T = [-inf, ..., 0 at n-1],
//     beta_t[j] = logaddexp(stay_t[j] + beta_{t+1}[j], move_t[j+1] + beta_{t+1}[j+1]);  logz = alpha_T[n-1];
//     p_stay[t][j] = exp(alpha_t[j]   + stay_t[j] + beta_{t+1}[j] - logz)
//     p_move[t][j] = exp(alpha_t[j-1] + move_t[j] + beta_{t+1}[j] - logz)
//     grad[n][t][c] (+)= weight[n] * (sum of p over the edges whose gathered score element is c).
//   In the koi layout the stay edge is the scalar blank_score: it has no element and gets no gradient.
//   One workgroup per chunk, one launch, the geometry of seq_scan_kernel. The forward pass is that kernel's Log scan - both are written
//   in the chain pieces of seq_chain.h, so logz is bit-identical to bh_crf_seq_logz by construction - and stores every alpha_t to the
//   workspace; each thread later reads back only what it wrote itself. The backward pass keeps beta in registers as the forward keeps alpha; thread `tid` scores the stay edge of its
//   positions and the move edge that LEAVES each of them, so the one value that crosses threads is move_t[j0] + beta_{t+1}[j0] of the
//   right neighbour's first position - by wave shift in the one-wave form, through LDS in the four-wave form.
//   REPEATED K-MERS. Several positions can gather the same score element at the same step (a homopolymer is the extreme case). A path takes
//   exactly one edge per step, so the posteriors of a step sum to 1: they are combined in a per-chunk LDS accumulator of unsigned 32-bit
//   fixed point at scale 2^30 (headroom 4) with integer atomics, whose result does not depend on arrival order. An owner table (LDS, the
//   smallest edge id that gathers the element, built once per chunk with an integer min) names the one thread that reads the sum, clears
//   the entry and does the single write of grad[t][c]. Every row of a chunk is written by that chunk's workgroup only: the result is
//   bit-identical from call to call. No floating-point atomic is used.
//   TARGET DOES NOT FIT (n - 1 > T): logz = -inf and the gradient is DEFINED as zero (nothing added, or zeros on overwrite). What koi does
//   there is unknown (it is closed); a NaN would poison an optimiser step and the +inf loss already flags the chunk. This is the project's
//   own definition, like the compact alignment form. Argument errors found on the device (len > Lmax, len < state_len): logz = NaN and
//   no gradient is written.
//   accumulate = 0: every element of the chunk's T rows is written exactly once (the elements no edge gathers get zeros).
//
// Dense gradient (bh_crf_logz_dense_grad): the posteriors of CTC_CRF.logZ, the mirror of crf_dense_logz_kernel. One thread per state;
//   the forward (the dense pieces of seq_chain.h, as in that kernel) stores alpha [T][S] in fp32, the backward keeps beta[s] in the register of thread s and passes the four
//   move_t[s'][r] + beta_{t+1}[s'] terms to the predecessor states through a double-buffered LDS table. Thread s' writes the 5 (4 in the
//   koi layout) elements of its state: every element of the chunk's rows exactly once, deterministic by construction.
//     grad[n][t][5s'+0]   = weight[n] * exp(alpha_t[s'] + stay_t[s'] + beta_{t+1}[s'] - logZ)
//     grad[n][t][5s'+1+r] = weight[n] * exp(alpha_t[r S/4 + s'/4] + move_t[s'][r] + beta_{t+1}[s'] - logZ)
#include <math.h>

#include "common.h"
#include "kernels.h"
#include "seq_chain.h"

namespace bh {
namespace {                                  // (file-local: args, kernels and their table)

constexpr int GU = 4;                        // prefetch depth (time steps), both directions (2 at 16 positions per thread: registers)
constexpr float FIX_ONE = 1073741824.0f;     // 2^30: fixed-point scale of the per-step posterior accumulator
constexpr int NO_OWNER = 0x7fffffff;

struct SeqGradArgs {
    ChainArgs c;
    const float* weight;         // [N] or null (= 1)
    float* alpha;                // [N][T][apitch]
    int apitch, C;
    float* out;                  // [N]
    void* grad;                  // fp16 or fp32, element strides g_n / g_t, the score axis dense
    long g_n, g_t;
    int g32, accumulate;
};

template <int P, bool MULTI>
__global__ __launch_bounds__(256) void seq_grad_kernel(SeqGradArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ChainArgs& ch = p.c;
    const int n = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, C = p.C, T = ch.T;
    const int len = ch.lens[n];
    const int npos = len + 1 - ch.k;
    if (len > ch.Lmax || npos <= 0) {                                        // argument error on the device: NaN and no gradient
        if (tid == 0) p.out[n] = __builtin_nanf("");
        return;
    }
    float* edge = (float*)smem;                                             // [2][NT] hand-off (MULTI)
    float* s_logz = edge + 2 * NT;                                          // [4]
    unsigned* acc = (unsigned*)(s_logz + 4);                                // [2][C] fixed-point posterior sums of a step
    int* own = (int*)(acc + 2 * C);                                         // [C] smallest edge id that gathers the element
    const bool g32 = p.g32 != 0, add = p.accumulate != 0;
    const long gbase = (long)n * p.g_n;

    // ---- the chain: gather offsets of this thread's positions, and of the move edge into the right neighbour's first ----
    int so[P], mo[P + 1];
#pragma unroll
    for (int i = 0; i <= P; ++i) {
        int s;
        chain_offsets(ch, n, tid * P + i, s, mo[i]);
        if (i < P) so[i] = s;
    }

    // ---- owner table: edge 2j = stay of position j (5S layout), edge 2j + 1 = move j -> j + 1; only edges of the chain's n positions ----
    for (int c = tid; c < C; c += NT) { own[c] = NO_OWNER; acc[c] = 0u; acc[C + c] = 0u; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int j = tid * P + i;
        if (ch.five && j < npos) atomicMin(&own[so[i]], 2 * j);
        if (j + 1 < npos) atomicMin(&own[mo[i + 1]], 2 * j + 1);
    }
    __syncthreads();
    unsigned own_s = 0, own_m = 0;                                          // bit i: this thread writes the element of its i-th stay / move edge
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int j = tid * P + i;
        if (ch.five && j < npos && own[so[i]] == 2 * j) own_s |= 1u << i;
        if (j + 1 < npos && own[mo[i + 1]] == 2 * j + 1) own_m |= 1u << i;
    }

    const half_t* sc = ch.scores + (long)n * ch.s_n;
    constexpr int U = P >= 16 ? 2 : GU;
    float sv[U][P], mv[U][P];
    float a[P];
#pragma unroll
    for (int i = 0; i < P; ++i) a[i] = -INFINITY;
    if (tid == 0) a[0] = 0.0f;
    const bool stores = tid * P < p.apitch;                                 // apitch is a multiple of P
    float* aw = p.alpha + ((long)n * T) * p.apitch + tid * P;
    int cb = 0;
    const bool fits = npos - 1 <= T;                                        // uniform

    // ---- forward: the Log scan of seq_scan_kernel; alpha_t (before step t) goes to the workspace ----
    if (fits) {
        auto load = [&](int slot, int t) {                                  // (rows beyond the end are never used)
            chain_load(ch, sc + (long)min(t, T - 1) * ch.s_t, so, mo, sv[slot], mv[slot]);
        };
#pragma unroll
        for (int u = 0; u < U; ++u) load(u, u);
        for (int t0 = 0; t0 < T; t0 += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u;
                if (t < T) {                                                // uniform across the workgroup
                    if (stores) {
#pragma unroll
                        for (int i = 0; i < P; ++i) aw[(long)t * p.apitch + i] = a[i];
                    }
                    chain_log_step(a, chain_from_left<MULTI>(a[P - 1], edge, cb, tid, NT), sv[u], mv[u]);
                    load(u, t + U);
                }
            }
        }
        const int last = npos - 1;
        if (last / P == tid) {
            float r = a[0];
#pragma unroll
            for (int i = 1; i < P; ++i)
                if (last % P == i) r = a[i];
            p.out[n] = r;
            s_logz[0] = r;
        }
    } else if (tid == 0) {
        p.out[n] = -INFINITY;
        s_logz[0] = -INFINITY;
    }
    __syncthreads();
    const float logz = s_logz[0];

    if (!(logz > -INFINITY)) {                                              // no alignment: the gradient is defined as zero
        if (!add)
            for (int t = 0; t < T; ++t)
                for (int c = tid; c < C; c += NT) grad_put(p.grad, gbase + (long)t * p.g_t + c, 0.0f, g32, false);
        return;
    }
    if (!add) {                                                             // the elements no edge gathers: zeros, each written once
        for (int c = tid; c < C; c += NT)
            if (own[c] == NO_OWNER)
                for (int t = 0; t < T; ++t) grad_put(p.grad, gbase + (long)t * p.g_t + c, 0.0f, g32, false);
    }
    const float w = (p.weight ? p.weight[n] : 1.0f) * (1.0f / FIX_ONE);

    // ---- backward: beta in registers; the sums of step t are written one barrier later, while step t - 1 is scored ----
    float av[U][P];
    auto loadb = [&](int slot, int t) {
        const int tt = max(t, 0);
        chain_load(ch, sc + (long)tt * ch.s_t, so, mo, sv[slot], mv[slot]);
#pragma unroll
        for (int i = 0; i < P; ++i) av[slot][i] = stores ? aw[(long)tt * p.apitch + i] : -INFINITY;
    };
    auto flush = [&](int t, int buf) {                                      // the owners of step t's elements: read, clear, one write each
        unsigned* ac = acc + buf * C;
        const long at = gbase + (long)t * p.g_t;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            if ((own_s >> i) & 1) {
                const unsigned v = ac[so[i]];
                ac[so[i]] = 0u;
                if (v || !add) grad_put(p.grad, at + so[i], w * (float)v, g32, add);
            }
            if ((own_m >> i) & 1) {
                const unsigned v = ac[mo[i + 1]];
                ac[mo[i + 1]] = 0u;
                if (v || !add) grad_put(p.grad, at + mo[i + 1], w * (float)v, g32, add);
            }
        }
    };
    float b[P];
#pragma unroll
    for (int i = 0; i < P; ++i) b[i] = (tid * P + i == npos - 1) ? 0.0f : -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) loadb(u, T - 1 - u);
    int buf = 0;
    for (int t0 = T - 1; t0 >= 0; t0 -= U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 - u;
            if (t >= 0) {                                                   // uniform across the workgroup
                const float x = mv[u][0] + b[0];                            // move_t[j0] + beta_{t+1}[j0] for the left neighbour
                if constexpr (!MULTI) __syncthreads();                      // (one wave: orders the accumulator, costs no wait on others)
                const float nxt = chain_from_right<MULTI>(x, edge, cb, tid, NT);
                if (t < T - 1) flush(t + 1, buf ^ 1);
                unsigned* ac = acc + buf * C;
#pragma unroll
                for (int i = 0; i < P; ++i) {                               // ascending: position i reads the OLD beta of i + 1
                    const float in = i + 1 < P ? mv[u][i + 1] + b[i + 1] : nxt;
                    const float st = sv[u][i] + b[i];
                    const float base = av[u][i] - logz;
                    if (ch.five) {
                        const unsigned q = (unsigned)(__expf(base + st) * FIX_ONE + 0.5f);
                        if (q) atomicAdd(&ac[so[i]], q);
                    }
                    const unsigned q = (unsigned)(__expf(base + in) * FIX_ONE + 0.5f);
                    if (q) atomicAdd(&ac[mo[i + 1]], q);
                    b[i] = lse2(st, in);
                }
                buf ^= 1;
                loadb(u, t - U);
            }
        }
    }
    __syncthreads();
    flush(0, buf ^ 1);
}

// ---- posteriors of CTC_CRF.logZ: one thread per state ---------------------------------------------------------------------------------
struct DenseGradArgs {
    const half_t* scores;
    int N, T, S, five;
    float blank;
    long s_n, s_t;
    const float* weight;         // [N] or null (= 1)
    float* alpha;                // [N][T][S]
    float* out;                  // [N]
    void* grad;
    long g_n, g_t;
    int g32;
};

__global__ __launch_bounds__(1024) void crf_dense_grad_kernel(DenseGradArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* al = (float*)smem;                                               // [2][S] forward ping-pong
    float* tm = al + 2 * p.S;                                               // [2][S][4] backward: move_t[s'][r] + beta_{t+1}[s']
    float* s_logz = tm + 8 * p.S;
    const int n = blockIdx.x, j = threadIdx.x, S = p.S, q = S >> 2;
    const bool active = j < S;
    const int W = p.five ? 5 : 4;
    const half_t* sc = p.scores + (long)n * p.s_n + W * (active ? j : 0);
    float* aw = p.alpha + (long)n * p.T * S;
    if (active) al[j] = 0.0f;
    __syncthreads();
    float ring[GU][5];
    auto load = [&](int slot, int t) { dense_load(p, sc + (long)max(0, min(t, p.T - 1)) * p.s_t, ring[slot]); };
    // ---- forward: crf_dense_logz_kernel, alpha_t (before step t) kept ----
    int cb = 0;
#pragma unroll
    for (int v = 0; v < GU; ++v) load(v, v);
    for (int t0 = 0; t0 < p.T; t0 += GU) {
#pragma unroll
        for (int v = 0; v < GU; ++v) {
            if (t0 + v < p.T) {                                             // uniform across the workgroup
                const float* a = al + cb * S;
                if (active) {
                    aw[(long)(t0 + v) * S + j] = a[j];
                    al[(cb ^ 1) * S + j] = dense_step(a, j, q, ring[v]);
                }
                cb ^= 1;
                __syncthreads();
                load(v, t0 + v + GU);
            }
        }
    }
    if (j == 0) {
        const float r = dense_final(al + cb * S, S);
        p.out[n] = r;
        s_logz[0] = r;
    }
    __threadfence();           // the alpha rows of this workgroup -> visible to its own later loads from other threads
    __syncthreads();
    __threadfence();
    const float logz = s_logz[0];
    const float w = p.weight ? p.weight[n] : 1.0f;

    // ---- backward ----
    float beta = 0.0f;
    float ar[GU][5];
    auto loadb = [&](int slot, int t) {
        load(slot, t);
        const float* a = aw + (long)max(t, 0) * S;
        ar[slot][0] = active ? a[j] : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) ar[slot][1 + r] = active ? a[r * q + (j >> 2)] : 0.0f;
    };
#pragma unroll
    for (int v = 0; v < GU; ++v) loadb(v, p.T - 1 - v);
    cb = 0;
    const long gbase = (long)n * p.g_n + W * (active ? j : 0);
    for (int t0 = p.T - 1; t0 >= 0; t0 -= GU) {
#pragma unroll
        for (int v = 0; v < GU; ++v) {
            const int t = t0 - v;
            if (t >= 0) {                                                   // uniform across the workgroup
                float* x = tm + cb * 4 * S;
                if (active) {
                    const long at = gbase + (long)t * p.g_t;
                    const float base = beta - logz;
                    if (p.five) {
                        const float g = w * __expf(ar[v][0] + ring[v][0] + base);
                        if (p.g32) ((float*)p.grad)[at] = g; else ((half_t*)p.grad)[at] = (half_t)g;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float g = w * __expf(ar[v][1 + r] + ring[v][1 + r] + base);
                        const long e = at + (p.five ? 1 : 0) + r;
                        if (p.g32) ((float*)p.grad)[e] = g; else ((half_t*)p.grad)[e] = (half_t)g;
                        x[4 * j + r] = ring[v][1 + r] + beta;
                    }
                }
                __syncthreads();
                if (active) {                                               // state j's successors (j % q) 4 + b hold j as predecessor r = j / q
                    float c[5];
                    c[0] = ring[v][0] + beta;
#pragma unroll
                    for (int bb = 0; bb < 4; ++bb) c[1 + bb] = x[4 * ((j % q) * 4 + bb) + j / q];
                    beta = lse_n(c);
                }
                cb ^= 1;
                loadb(v, t - GU);
            }
        }
    }
}

// the gradient kernels of the instance list, in its order
typedef void (*SeqGradKernel)(SeqGradArgs);
#define BH_SEQ_GRAD_ROW(NT, P, MULTI) seq_grad_kernel<P, MULTI>,
const SeqGradKernel kSeqGradKernels[] = {BH_SEQ_INSTANCES(BH_SEQ_GRAD_ROW)};
#undef BH_SEQ_GRAD_ROW

int alpha_pitch(int Lmax, int k, int P) {                                   // positions kept per step: the chain, rounded up to whole threads
    int pm = Lmax + 1 - k;
    if (pm < 1) pm = 1;
    return (pm + P - 1) / P * P;
}

}  // namespace
}  // namespace bh

size_t bh_k_crf_seq_grad_workspace(int N, int T, int Lmax, int state_len) {
    if (N <= 0 || T <= 0 || Lmax < 0 || state_len < 1 || state_len > 5) return 0;
    const int row = bh::chain_instance(Lmax, state_len);
    if (row < 0) return 0;
    return (size_t)N * T * bh::alpha_pitch(Lmax, state_len, bh::kSeqGeometry[row].per) * sizeof(float) + 512;
}

int bh_k_crf_seq_grad(const void* scores, int N, int T, int state_len, int layout_5s, float blank, long s_n, long s_t,
                      const void* targets, int target_bytes, int Lmax, const int* lens, const float* weight, void* workspace,
                      float* out, void* grad, long g_n, long g_t, int grad_fp32, int accumulate, hipStream_t stream) {
    using namespace bh;
    if (int rc = chain_check("crf_seq_grad", state_len, N, T, layout_5s, target_bytes, Lmax, state_len)) return rc;
    BH_REQUIRE((grad_fp32 == 0 || grad_fp32 == 1) && (accumulate == 0 || accumulate == 1), "crf_seq_grad: flags must be 0 or 1");
    int row;
    if (int rc = chain_instance_check("crf_seq_grad", Lmax, state_len, &row)) return rc;
    const int threads = kSeqGeometry[row].threads, P = kSeqGeometry[row].per;
    const int C = (layout_5s ? 5 : 4) << (2 * state_len);
    SeqGradArgs a{{(const half_t*)scores, N, T, state_len, layout_5s, blank, s_n, s_t, targets, target_bytes, Lmax, lens}, weight,
                  (float*)workspace, alpha_pitch(Lmax, state_len, P), C, out, grad, g_n, g_t, grad_fp32, accumulate};
    const size_t lds = (2 * threads + 4) * sizeof(float) + (size_t)3 * C * sizeof(int);
    hipLaunchKernelGGL(kSeqGradKernels[row], dim3(N), dim3(threads), lds, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

size_t bh_k_crf_logz_dense_grad_workspace(int N, int T, int state_len) {
    if (N <= 0 || T <= 0 || state_len < 1 || state_len > 5) return 0;
    return ((size_t)N * T << (2 * state_len)) * sizeof(float) + 512;
}

int bh_k_crf_logz_dense_grad(const void* scores, int N, int T, int state_len, int layout_5s, float blank, long s_n, long s_t,
                             const float* weight, void* workspace, float* out, void* grad, long g_n, long g_t, int grad_fp32,
                             hipStream_t stream) {
    using namespace bh;
    if (int rc = dense_check("crf_logz_dense_grad", state_len, N, T, layout_5s)) return rc;
    BH_REQUIRE(grad_fp32 == 0 || grad_fp32 == 1, "crf_logz_dense_grad: grad_fp32 must be 0 or 1 (got %d)", grad_fp32);
    const int S = 1 << (2 * state_len);
    DenseGradArgs a{(const half_t*)scores, N, T, S, layout_5s, blank, s_n, s_t, weight, (float*)workspace, out, grad, g_n, g_t,
                    grad_fp32};
    hipLaunchKernelGGL(crf_dense_grad_kernel, dim3(N), dim3(S < 64 ? 64 : S), (size_t)(10 * S + 4) * sizeof(float), stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
