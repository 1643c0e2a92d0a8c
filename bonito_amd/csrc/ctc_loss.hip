// The CTC loss of bonito.ctc on gfx950: what Model.ctc_label_smoothing_loss (reference bonito/ctc/model.py:48-57) takes from
// torch.nn.functional.ctc_loss, with its gradient and the numerator of the label-smoothing term, from ONE launch.
//
// Definition (torch's, blank = class 0). l' = the target with blanks interleaved, S = 2 len + 1 states, lp_t = row t of log_probs:
//     alpha_0[0] = lp_0[0], alpha_0[1] = lp_0[l'_1];
//     alpha_t[s] = lp_t[l'_s] + logsumexp(alpha_{t-1}[s], alpha_{t-1}[s-1], alpha_{t-1}[s-2]),  the s-2 term only when l'_s != 0 and
//                  l'_s != l'_{s-2};            nll = -logaddexp(alpha_{T-1}[S-1], alpha_{T-1}[S-2]);
//     beta = the mirror scan;  occ[t][c] = sum over the states s with l'_s = c of P(the path is in s at step t | target).
//   Outputs per chunk: nll[n]; smooth[n] = sum_t sum_c w_c lp[t][n][c] (w = a device float[C] or null: not computed; classes with
//   w_c = 0 are left out of the sum); and in the gradient entry point  grad[t][n][c] (+)= -weight[n] occ[t][c] + smooth_weight[n] w_c.
//   THE GRADIENT IS THE TRUE DERIVATIVE of nll with respect to log_probs, -occ. torch's native kernel returns exp(lp) - occ (the
//   derivative with respect to the logits in front of a log_softmax); the two agree after log_softmax's backward.
//   This project's definitions where torch yields NaN:
//     * a target that cannot fit (len + adjacent repeats > T), or one every alignment of which crosses a -inf log-prob: nll = +inf
//       and a ZERO gradient (nothing added, or zeros on overwrite; the smoothing term is left out too) - the choice of seqdist_grad.hip;
//     * a state that a -inf log-prob makes unreachable contributes occupancy 0;
//     * len < 0, len > Lmax or a label outside 1..C-1: nll = NaN and no gradient is written.
//
// One workgroup per chunk, the instance list of seq_chain.h (which also holds lse2, the label read and grad_put): thread `tid` owns the P consecutive states tid P .. tid P + P - 1 in
// registers. With an even P the blank / label pattern of a thread's states is known at compile time, a blank never takes the s-2 term,
// and ONE value crosses a thread boundary forwards (alpha[s-1] of the left neighbour's last state; the one-state-per-thread instance
// passes s-2 as well) and two backwards - by wave shift in the one-wave form, through a double-buffered LDS table in the four-wave
// form. The forward stores every alpha_t in fp32 to the workspace and a thread later reads back only what it wrote; the backward keeps
// beta in registers. Rows are gathered U steps ahead.
//   THE CLASS SUMS. All len + 1 blank states gather class 0, so a step's occupancies are reduced per thread (integer fixed point at
//   scale 2^30: a step's occupancies sum to 1, headroom 4), then across the wave (a reduce-scatter of 10 exchanges that leaves class c
//   in lane 8c), and then combined ONCE per wave and class: the one-wave form writes the row from the wave sum, the four-wave form
//   stores its wave sums to an LDS slot of its own (no atomic at all) and threads 0..C-1 add the four slots one barrier later. Integer sums do not depend on the order: the result is bit-identical
//   from call to call. accumulate = 0: every element of the chunk's T rows is written exactly once.
#include <math.h>

#include "common.h"
#include "kernels.h"
#include "seq_chain.h"

namespace bh {
namespace {

constexpr float CTC_FIX_ONE = 1073741824.0f;     // 2^30
constexpr int CTC_MAX_C = 8;

struct CtcArgs {
    const void* lp;              // fp16 or fp32, element strides s_t / s_n, the class axis dense
    int lp32, N, T, C;
    long s_t, s_n;
    const void* targets;         // [N][Lmax] int8 or int32, labels 1..C-1, 0 = padding
    int tbytes, Lmax;
    const int* lens;             // [N]
    const float* sw;             // [C] or null
    const float* weight;         // [N] or null (= 1)
    const float* smooth_weight;  // [N] or null (= 0)
    float* alpha;                // [N][T][apitch]
    int apitch;
    float* nll;                  // [N]
    float* smooth;               // [N] or null
    void* grad;
    long g_t, g_n;
    int g32, accumulate;
};

__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);
    return m == -INFINITY ? m : m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}
__device__ __forceinline__ float ctc_ld(const CtcArgs& p, long at) {
    return p.lp32 ? ((const float*)p.lp)[at] : (float)((const half_t*)p.lp)[at];
}
__device__ __forceinline__ int ctc_target(const CtcArgs& p, int n, int len, int j) {      // label j of the chunk; 0 outside the target
    if (j < 0 || j >= len) return 0;
    return label_at(p.targets, p.tbytes, (long)n * p.Lmax + j);
}

// P states per thread; MULTI: four waves; GRAD: the backward pass; CM: the class sums kept per thread (C <= CM)
template <int P, bool MULTI, bool GRAD, int CM>
__global__ __launch_bounds__(256) void ctc_loss_kernel(CtcArgs p) {
    constexpr int NTMAX = MULTI ? 256 : 64;
    constexpr int U = P >= 16 ? 2 : 4;                                      // prefetch depth (time steps), both directions
    __shared__ float edge[MULTI ? 2 * NTMAX * 2 : 2];                       // [2][NT][2] hand-off
    __shared__ double red[4];
    __shared__ float s_end[2];
    __shared__ unsigned wsum[2 * 4 * CTC_MAX_C];                            // [2][wave][class] fixed-point occupancy sums of a step
    __shared__ int s_bad;
    const int n = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, C = p.C, T = p.T;
    const int lane = tid & 63, wave = tid >> 6;
    const int len = p.lens[n];
    const long base = (long)n * p.s_n;

    // ---- smooth[n]: the numerator of the label-smoothing term, fp64 partial sums combined in a fixed order ----
    if (p.smooth) {
        double acc = 0.0;
        const int total = T * C;
        for (int e = tid; e < total; e += NT) {
            const int t = e / C, c = e - t * C;
            const float w = p.sw[c];
            if (w != 0.0f) acc += (double)w * (double)ctc_ld(p, base + (long)t * p.s_t + c);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d);
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        if (tid == 0) {
            double s = red[0];
            for (int w = 1; w < NT / 64; ++w) s += red[w];
            p.smooth[n] = (float)s;
        }
    }
    if (len < 0 || len > p.Lmax) {                                          // argument error on the device: NaN and no gradient
        if (tid == 0) p.nll[n] = __builtin_nanf("");
        return;
    }
    if (tid == 0) { s_bad = 0; s_end[0] = -INFINITY; s_end[1] = -INFINITY; }
    __syncthreads();

    // ---- the states of this thread: class, validity, and whether the s-2 (forward) / s+2 (backward) term is allowed ----
    const int S = 2 * len + 1;
    int off[P];
    unsigned vmask = 0, fmask = 0, gmask = 0;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int s = tid * P + i;
        const bool lbl = (P % 2 == 0) ? (i & 1) != 0 : (s & 1) != 0;
        off[i] = 0;
        if (s < S) vmask |= 1u << i;
        if (lbl) {
            const int j = (s - 1) >> 1;
            const int lab = ctc_target(p, n, len, j);
            if (j < len) {
                if (lab < 1 || lab >= C) bad = true;
                off[i] = lab < 1 ? 0 : (lab >= C ? 0 : lab);
                if (j >= 1 && ctc_target(p, n, len, j - 1) != lab) fmask |= 1u << i;
                if (j + 1 < len && ctc_target(p, n, len, j + 1) != lab) gmask |= 1u << i;
            }
        }
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {
        if (tid == 0) p.nll[n] = __builtin_nanf("");
        return;
    }

    float lv[U][P];
    auto load = [&](int slot, int t) {                                      // (rows beyond either end are never used)
        const long row = base + (long)max(0, min(t, T - 1)) * p.s_t;
        const float b0 = ctc_ld(p, row);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const bool lbl = (P % 2 == 0) ? (i & 1) != 0 : true;
            const float v = lbl ? ctc_ld(p, row + off[i]) : b0;
            lv[slot][i] = (vmask >> i) & 1 ? v : -INFINITY;
        }
    };
    float a[P];
#pragma unroll
    for (int i = 0; i < P; ++i) a[i] = -INFINITY;
    if (tid == 0) a[0] = 0.0f;                                              // "alpha_{-1}": the first step then yields alpha_0
    const bool stores = GRAD && tid * P < p.apitch;                         // apitch is a multiple of P
    float* aw = GRAD ? p.alpha + ((long)n * T) * p.apitch + tid * P : nullptr;
    int cb = 0;

    // ---- forward: alpha_t goes to the workspace ----
#pragma unroll
    for (int u = 0; u < U; ++u) load(u, u);
    for (int t0 = 0; t0 < T; t0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u;
            if (t < T) {                                                    // uniform across the workgroup
                float prev1, prev2 = -INFINITY;
                if constexpr (MULTI) {
                    edge[(cb * NT + tid) * 2] = a[P - 1];
                    __syncthreads();
                    prev1 = tid ? edge[(cb * NT + tid - 1) * 2] : -INFINITY;
                    cb ^= 1;
                } else {
                    prev1 = __shfl_up(a[P - 1], 1);
                    if (tid < 1) prev1 = -INFINITY;
                    if constexpr (P == 1) {
                        prev2 = __shfl_up(a[0], 2);
                        if (tid < 2) prev2 = -INFINITY;
                    }
                }
#pragma unroll
                for (int i = P - 1; i >= 0; --i) {                          // descending: state i reads the OLD alpha of i - 1, i - 2
                    const float x1 = i >= 1 ? a[i - 1] : prev1;
                    const float x2 = i >= 2 ? a[i - 2] : (i == 1 ? prev1 : prev2);
                    const bool lbl = (P % 2 == 0) ? (i & 1) != 0 : true;
                    const float m = lbl ? ctc_lse3(a[i], x1, (fmask >> i) & 1 ? x2 : -INFINITY) : lse2(a[i], x1);
                    a[i] = lv[u][i] + m;
                }
                if (stores) {
#pragma unroll
                    for (int i = 0; i < P; ++i) aw[(long)t * p.apitch + i] = a[i];
                }
                load(u, t + U);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int s = tid * P + i;
        if (s == S - 1) s_end[0] = a[i];
        if (s == S - 2) s_end[1] = a[i];
    }
    __syncthreads();
    const float logz = lse2(s_end[0], s_end[1]);
    if (tid == 0) p.nll[n] = -logz;
    if constexpr (!GRAD) return;

    const bool g32 = p.g32 != 0, add = p.accumulate != 0;
    const long gbase = (long)n * p.g_n;
    if (!(logz > -INFINITY)) {                                              // no alignment: the gradient is defined as zero
        if (!add)
            for (int e = tid; e < T * C; e += NT) {
                const int t = e / C, c = e - t * C;
                grad_put(p.grad, gbase + (long)t * p.g_t + c, 0.0f, g32, false);
            }
        return;
    }
    const float w = -(p.weight ? p.weight[n] : 1.0f) * (1.0f / CTC_FIX_ONE);
    // who writes a step's row: the one-wave form from the wave sum (lane 8c holds class c, see below), the four-wave form threads 0..C-1
    const int wc = MULTI ? tid : lane >> 3;
    const bool writer = MULTI ? tid < C : ((lane & 7) == 0 && wc < C);
    const float swc = (p.smooth_weight && p.sw && writer) ? p.smooth_weight[n] * p.sw[wc] : 0.0f;

    // ---- backward: beta in registers; b' = the log-sum over the successors, occ = exp(alpha_t + b' - logz), beta_t = lp_t + b' ----
    float av[U][P];
    auto loadb = [&](int slot, int t) {
        load(slot, t);
        const int tt = max(t, 0);
#pragma unroll
        for (int i = 0; i < P; ++i) av[slot][i] = stores ? aw[(long)tt * p.apitch + i] : -INFINITY;
    };
    auto flush = [&](int t, int buf) {                                      // MULTI: threads 0..C-1 add the four wave sums of step t
        if (tid < C) {
            const unsigned* q = wsum + buf * 4 * CTC_MAX_C + tid;
            const unsigned v = q[0] + q[CTC_MAX_C] + q[2 * CTC_MAX_C] + q[3 * CTC_MAX_C];
            grad_put(p.grad, gbase + (long)t * p.g_t + tid, w * (float)v + swc, g32, add);
        }
    };
    float b[P];
#pragma unroll
    for (int i = 0; i < P; ++i) b[i] = (tid * P + i == S - 1) ? 0.0f : -INFINITY;     // "beta_T": the first step then yields b'_{T-1}
#pragma unroll
    for (int u = 0; u < U; ++u) loadb(u, T - 1 - u);
    int buf = 0;
    for (int t0 = T - 1; t0 >= 0; t0 -= U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 - u;
            if (t >= 0) {                                                   // uniform across the workgroup
                float nxt1, nxt2;
                if constexpr (MULTI) {
                    edge[(cb * NT + tid) * 2] = b[0];
                    edge[(cb * NT + tid) * 2 + 1] = b[P > 1 ? 1 : 0];
                    __syncthreads();
                    nxt1 = tid + 1 < NT ? edge[(cb * NT + tid + 1) * 2] : -INFINITY;
                    nxt2 = tid + 1 < NT ? edge[(cb * NT + tid + 1) * 2 + 1] : -INFINITY;
                    cb ^= 1;
                    if (t < T - 1) flush(t + 1, buf ^ 1);
                } else {
                    nxt1 = __shfl_down(b[0], 1);
                    if (tid >= NT - 1) nxt1 = -INFINITY;
                    if constexpr (P == 1) {
                        nxt2 = __shfl_down(b[0], 2);
                        if (tid >= NT - 2) nxt2 = -INFINITY;
                    } else {
                        nxt2 = __shfl_down(b[P > 1 ? 1 : 0], 1);
                        if (tid >= NT - 1) nxt2 = -INFINITY;
                    }
                }
                unsigned cs[CM];
#pragma unroll
                for (int c = 0; c < CM; ++c) cs[c] = 0u;
#pragma unroll
                for (int i = 0; i < P; ++i) {                               // ascending: state i reads the OLD beta of i + 1, i + 2
                    const float y1 = i + 1 < P ? b[i + 1 < P ? i + 1 : 0] : nxt1;
                    const float y2 = i + 2 < P ? b[i + 2 < P ? i + 2 : 0] : (i + 2 == P ? nxt1 : nxt2);
                    const bool lbl = (P % 2 == 0) ? (i & 1) != 0 : true;
                    const float m = lbl ? ctc_lse3(b[i], y1, (gmask >> i) & 1 ? y2 : -INFINITY) : lse2(b[i], y1);
                    const unsigned q = (unsigned)(__expf(av[u][i] + m - logz) * CTC_FIX_ONE + 0.5f);
                    if (lbl) {
#pragma unroll
                        for (int c = 0; c < CM; ++c) cs[c] += off[i] == c ? q : 0u;       // (a blank state of P = 1 has off = 0)
                    } else {
                        cs[0] += q;
                    }
                    b[i] = lv[u][i] + m;
                }
                // the wave sum as a reduce-scatter (10 exchanges in place of 6 per class): each of the first three exchanges halves
                // the classes a lane carries - the lanes with the bit set keep the upper half - so lane l ends with class (l >> 3) & 7,
                // summed over the 8 lanes that share those bits by the last three
                unsigned r4[4], r2[2];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned lo = k < CM ? cs[k < CM ? k : 0] : 0u, hi = k + 4 < CM ? cs[k + 4 < CM ? k + 4 : 0] : 0u;
                    r4[k] = ((lane & 32) ? hi : lo) + __shfl_xor((lane & 32) ? lo : hi, 32);
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) r2[k] = ((lane & 16) ? r4[k + 2] : r4[k]) + __shfl_xor((lane & 16) ? r4[k] : r4[k + 2], 16);
                unsigned mine = ((lane & 8) ? r2[1] : r2[0]) + __shfl_xor((lane & 8) ? r2[0] : r2[1], 8);
                mine += __shfl_xor(mine, 4);
                mine += __shfl_xor(mine, 2);
                mine += __shfl_xor(mine, 1);
                if constexpr (MULTI) {
                    if ((lane & 7) == 0) wsum[(buf * 4 + wave) * CTC_MAX_C + (lane >> 3)] = mine;
                    buf ^= 1;
                } else {
                    if (writer) grad_put(p.grad, gbase + (long)t * p.g_t + wc, w * (float)mine + swc, g32, add);
                }
                loadb(u, t - U);
            }
        }
    }
    if constexpr (MULTI) {
        __syncthreads();
        flush(0, buf ^ 1);
    }
}

// the kernels of the instance list (seq_chain.h), in its order; the first row that holds 2 Lmax + 1 states serves the call.
// id: enum bh_ctc_loss_kernel = the states per thread, + 100 in the four-wave form
typedef void (*CtcKernel)(CtcArgs);
struct CtcKernels { int id; CtcKernel fwd, grad5, grad8; };
#define BH_CTC_ROW(NT, P, MULTI) \
    {(MULTI ? 100 : 0) + P, ctc_loss_kernel<P, MULTI, false, 5>, ctc_loss_kernel<P, MULTI, true, 5>, ctc_loss_kernel<P, MULTI, true, 8>},
const CtcKernels kCtcKernels[] = {BH_SEQ_INSTANCES(BH_CTC_ROW)};
#undef BH_CTC_ROW
static_assert(BH_CTC_LOSS_K_W1 == 1 && BH_CTC_LOSS_K_W8 == 8 && BH_CTC_LOSS_K_M4 == 104 && BH_CTC_LOSS_K_M16 == 116, "instance codes");

int ctc_instance(int Lmax) { return Lmax < 0 ? -1 : seq_instance(2 * (long)Lmax + 1); }

int g_ctc_loss_last_kernel = 0;    // bh_k_ctc_loss_last_kernel (test hook, not thread-safe)

}  // namespace
}  // namespace bh

int bh_k_ctc_loss_last_kernel() { return bh::g_ctc_loss_last_kernel; }

size_t bh_k_ctc_loss_workspace(int N, int T, int C, int Lmax, int grad) {
    if (N <= 0 || T <= 0 || C < 2 || C > bh::CTC_MAX_C || Lmax > 2047) return 0;
    const int row = bh::ctc_instance(Lmax);
    if (row < 0) return 0;
    if (!grad) return 512;                                                  // the forward keeps nothing
    const int S = 2 * Lmax + 1, per = bh::kSeqGeometry[row].per;
    return (size_t)N * T * ((S + per - 1) / per * per) * sizeof(float) + 512;
}

int bh_k_ctc_loss(const void* log_probs, int logp_fp32, int N, int T, int C, long s_t, long s_n, const void* targets, int target_bytes,
                  int Lmax, const int* lens, const float* smooth_w, const float* weight, const float* smooth_weight, void* workspace,
                  float* nll, float* smooth, void* grad, long g_t, long g_n, int grad_fp32, int accumulate, int with_grad,
                  hipStream_t stream) {
    using namespace bh;
    const char* who = with_grad ? "ctc_loss_grad" : "ctc_loss";
    BH_REQUIRE(log_probs && lens && nll && workspace && (targets || Lmax == 0), "%s: null pointer", who);
    BH_REQUIRE(!with_grad || grad, "%s: null pointer", who);
    BH_REQUIRE(!smooth || smooth_w, "%s: smooth_out needs smooth_w", who);
    BH_REQUIRE(!smooth_weight || smooth_w, "%s: smooth_weight needs smooth_w", who);
    BH_REQUIRE(C >= 2 && C <= CTC_MAX_C, "%s: C must be in 2..8 (got %d)", who, C);
    BH_REQUIRE(N > 0 && T > 0, "%s: empty problem N=%d T=%d", who, N, T);
    BH_REQUIRE(Lmax >= 0 && Lmax <= 2047, "%s: Lmax must be in 0..2047 (got %d)", who, Lmax);
    BH_REQUIRE(target_bytes == 1 || target_bytes == 4, "%s: targets must be int8 or int32 (target_bytes %d)", who, target_bytes);
    BH_REQUIRE(logp_fp32 == 0 || logp_fp32 == 1, "%s: logp_fp32 must be 0 or 1 (got %d)", who, logp_fp32);
    BH_REQUIRE((T == 1 || s_t >= C) && (N == 1 || s_n >= C), "%s: bad strides (stride_t %ld, stride_n %ld) for %d dense classes", who,
               s_t, s_n, C);
    if (with_grad) {
        BH_REQUIRE((grad_fp32 == 0 || grad_fp32 == 1) && (accumulate == 0 || accumulate == 1), "%s: flags must be 0 or 1", who);
        const bool tn = (N == 1 || g_n >= C) && (T == 1 || g_t >= (long)(N - 1) * g_n + C);      // [T][N][C]-like
        const bool nt = (T == 1 || g_t >= C) && (N == 1 || g_n >= (long)(T - 1) * g_t + C);      // [N][T][C]-like
        BH_REQUIRE(tn || nt, "%s: bad strides (g_stride_t %ld, g_stride_n %ld): the rows of grad overlap", who, g_t, g_n);
    }
    const int row = ctc_instance(Lmax);
    BH_REQUIRE(row >= 0, "%s: no instance for Lmax %d", who, Lmax);
    const CtcKernels& r = kCtcKernels[row];
    const int S = 2 * Lmax + 1, per = kSeqGeometry[row].per;
    CtcArgs a{log_probs, logp_fp32, N, T, C, s_t, s_n, targets, target_bytes, Lmax, lens, smooth_w, weight, smooth_weight,
              (float*)workspace, (S + per - 1) / per * per, nll, smooth, grad, g_t, g_n, grad_fp32, accumulate};
    const CtcKernel fn = !with_grad ? r.fwd : (C <= 5 ? r.grad5 : r.grad8);
    hipLaunchKernelGGL(fn, dim3(N), dim3(kSeqGeometry[row].threads), 0, stream, a);
    g_ctc_loss_last_kernel = r.id;
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
