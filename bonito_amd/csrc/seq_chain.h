// What the sequence scans share: seqdist.hip (the CTC-CRF Log scan, Max scan, free start and dense logZ), seqdist_grad.hip (their
// alpha-beta gradients) and ctc_loss.hip (the CTC loss of bonito.ctc). Each piece is written ONCE here and the kernels of the three
// files are written in terms of them: the gradient entry points promise a logz that is bit-identical to the plain scans', and they
// keep that promise because both run this code, not two copies of it.
//
// Device code: lse2 / lse_n, the label read, grad_put, the chain (one problem description, gather offsets, ring load, neighbour
// hand-offs, Log-scan step) and the dense scan (ring load, step, final log-sum). Host code: the (threads, positions per thread)
// instance list with its one look-up, and the argument checks the paired entry points share.
#pragma once
#include <math.h>

#include "common.h"

namespace bh {

// ---- log-sums ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b), d = fminf(a, b) - m;
    return m == -INFINITY ? m : m + __logf(1.0f + __expf(d));
}

// log of the sum of exp over a small register array: the max first, then the sum in index order. GUARD: the array may be -inf
// throughout (the max then starts from -inf and an all -inf array yields -inf); without it the caller knows c[0] is finite
template <bool GUARD = false, int N>
__device__ __forceinline__ float lse_n(const float (&c)[N]) {
    float m = GUARD ? -INFINITY : c[0];
#pragma unroll
    for (int i = GUARD ? 0 : 1; i < N; ++i) m = fmaxf(m, c[i]);
    if (GUARD && m == -INFINITY) return m;
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) sum += __expf(c[i] - m);
    return m + __logf(sum);
}

// ---- labels and gradient elements -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int label_at(const void* targets, int tbytes, long at) {      // int8 or int32 rows
    return tbytes == 1 ? (int)((const int8_t*)targets)[at] : ((const int*)targets)[at];
}

__device__ __forceinline__ void grad_put(void* g, long at, float v, bool g32, bool add) {
    if (g32) {
        float* q = (float*)g + at;
        *q = add ? *q + v : v;
    } else {
        half_t* q = (half_t*)g + at;
        *q = (half_t)(add ? (float)*q + v : v);
    }
}

// ---- the chain of CTC_CRF.prepare_ctc_scores (see seqdist.hip) --------------------------------------------------------------------
struct ChainArgs {
    const half_t* scores;
    int N, T, k, five;
    float blank;
    long s_n, s_t;
    const void* targets;         // [N][Lmax] int8 or int32
    int tbytes, Lmax;
    const int* lens;             // [N]
};

__device__ __forceinline__ int target0(const ChainArgs& c, int n, int i) {                // targets0[i]; 0 beyond the row
    if (i >= c.Lmax) return 0;
    const int v = label_at(c.targets, c.tbytes, (long)n * c.Lmax + i) - 1;
    return v < 0 ? 0 : (v > 3 ? 3 : v);
}

// gather offsets of chain position j: the stay element (5S layout) and the move edge INTO j (for j = 0 an edge no path takes). The loop
// over a thread's positions stays in the kernels: with the loop inside the helper the compiler arranged the prologue differently and the
// Log and Max scans measured 0.3 - 0.7 % slower
__device__ __forceinline__ void chain_offsets(const ChainArgs& c, int n, int j, int& so, int& mo) {
    int kmer = 0;
    for (int d = 0; d < c.k; ++d) kmer = kmer * 4 + target0(c, n, j + d);
    const int b = j > 0 ? target0(c, n, j - 1) : 0;
    so = 5 * kmer;
    mo = c.five ? 5 * kmer + 1 + b : 4 * kmer + b;
}

// one slot of the register ring: the stay and move values of score row `row` (the caller clamps the step into 0 .. T - 1)
template <int P, int NM>
__device__ __forceinline__ void chain_load(const ChainArgs& c, const half_t* row, const int (&so)[P], const int (&mo)[NM], float (&sv)[P],
                                           float (&mv)[P]) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
        sv[i] = c.five ? (float)row[so[i]] : c.blank;
        mv[i] = (float)row[mo[i]];
    }
}

// the one value that crosses threads, `x` of the left / right neighbour (-inf at the end of the chunk): by wave shift in the one-wave
// form - no LDS, no barrier - and through edge[2][NT] with one barrier in the four-wave form (cb: the buffer of this step)
template <bool MULTI>
__device__ __forceinline__ float chain_from_left(float x, float* edge, int& cb, int tid, int NT) {
    float prev;
    if constexpr (MULTI) {
        edge[cb * NT + tid] = x;
        __syncthreads();
        prev = tid ? edge[cb * NT + tid - 1] : -INFINITY;
        cb ^= 1;
    } else {
        prev = __shfl_up(x, 1);
        if (tid == 0) prev = -INFINITY;
    }
    return prev;
}

template <bool MULTI>
__device__ __forceinline__ float chain_from_right(float x, float* edge, int& cb, int tid, int NT) {
    float nxt;
    if constexpr (MULTI) {
        edge[cb * NT + tid] = x;
        __syncthreads();
        nxt = tid + 1 < NT ? edge[cb * NT + tid + 1] : -INFINITY;
        cb ^= 1;
    } else {
        nxt = __shfl_down(x, 1);
        if (tid == NT - 1) nxt = -INFINITY;
    }
    return nxt;
}

// one step of the Log scan over a thread's positions; prev = the left neighbour's last alpha
template <int P>
__device__ __forceinline__ void chain_log_step(float (&a)[P], float prev, const float (&sv)[P], const float (&mv)[P]) {
#pragma unroll
    for (int i = P - 1; i >= 0; --i) {                                      // descending: position i reads the OLD alpha of i - 1
        const float in = (i ? a[i - 1] : prev) + mv[i];
        const float st = a[i] + sv[i];
        a[i] = lse2(st, in);
    }
}

// (The pick of alpha_T[npos - 1] from a thread's registers stays written out in the two chain kernels: as a function of the array the
// compiler folds its compare chain into ONE indexed read before it is inlined, and an indexed array cannot live in registers - every
// instance with P >= 4 then kept alpha in scratch or LDS.)

// ---- the dense scan of CTC_CRF.logZ: one thread per state j, alpha in LDS ---------------------------------------------------------
// one slot of the ring: the stay score and the four move scores of a state, `row` pointing at the state's elements. p = the kernel's
// DenseArgs / DenseGradArgs (five, blank), read through the struct as the kernels always did: passed by value the two cost ~60 more
// scalar instructions per kernel
template <class Args>
__device__ __forceinline__ void dense_load(const Args& p, const half_t* row, float (&ring)[5]) {
    ring[0] = p.five ? (float)row[0] : p.blank;
#pragma unroll
    for (int r = 0; r < 4; ++r) ring[1 + r] = (float)row[(p.five ? 1 : 0) + r];
}

// the new alpha of state j of S = 4 q states from the alphas `a` of the step before
__device__ __forceinline__ float dense_step(const float* a, int j, int q, const float (&ring)[5]) {
    float c[5];
    c[0] = a[j] + ring[0];
#pragma unroll
    for (int r = 0; r < 4; ++r) c[1 + r] = a[r * q + (j >> 2)] + ring[1 + r];
    return lse_n(c);
}

__device__ __forceinline__ float dense_final(const float* a, int S) {                     // the log-sum over the S states
    float m = a[0];
    for (int i = 1; i < S; ++i) m = fmaxf(m, a[i]);
    float sum = 0.0f;
    for (int i = 0; i < S; ++i) sum += __expf(a[i] - m);
    return m + __logf(sum);
}

// ---- host side: THE instance list ------------------------------------------------------------------------------------------------
// X(threads, positions per thread, four waves): a row serves up to threads x per positions (CTC loss: states). Each file makes its
// table of kernel pointers from this list; a new width is added here and nowhere else.
#define BH_SEQ_INSTANCES(X) \
    X(64, 1, false) X(64, 2, false) X(64, 4, false) X(64, 8, false) X(256, 4, true) X(256, 8, true) X(256, 16, true)

struct SeqGeometry { int threads, per; };
#define BH_SEQ_GEOMETRY_ROW(NT, P, MULTI) {NT, P},
constexpr SeqGeometry kSeqGeometry[] = {BH_SEQ_INSTANCES(BH_SEQ_GEOMETRY_ROW)};
#undef BH_SEQ_GEOMETRY_ROW

inline int seq_instance(long positions) {                                  // the first row that holds this many positions, else -1
    for (int i = 0; i < (int)(sizeof(kSeqGeometry) / sizeof(kSeqGeometry[0])); ++i)
        if (positions <= (long)kSeqGeometry[i].threads * kSeqGeometry[i].per) return i;
    return -1;
}

inline int chain_instance(int Lmax, int k) {                               // ... for the chain of rows of up to Lmax labels
    const int pm = Lmax + 1 - k;
    return seq_instance(pm < 1 ? 1 : pm);
}

// ---- host side: the argument checks a plain entry point and its gradient twin share; `who` names the entry point in the messages --
inline int chain_check(const char* who, int state_len, int N, int T, int layout_5s, int target_bytes, int Lmax, int Lmin) {
    BH_REQUIRE(state_len >= 1 && state_len <= 5, "%s: state_len must be in 1..5 (got %d)", who, state_len);
    BH_REQUIRE(N > 0 && T > 0, "%s: empty problem N=%d T=%d", who, N, T);
    BH_REQUIRE(layout_5s == 0 || layout_5s == 1, "%s: layout_5s must be 0 or 1 (got %d)", who, layout_5s);
    BH_REQUIRE(target_bytes == 1 || target_bytes == 4, "%s: targets must be int8 or int32 (target_bytes %d)", who, target_bytes);
    BH_REQUIRE(Lmax >= Lmin, "%s: rows of %d labels are shorter than state_len %d", who, Lmax, state_len);
    return 0;
}

inline int chain_instance_check(const char* who, int Lmax, int state_len, int* row) {
    *row = chain_instance(Lmax, state_len);
    BH_REQUIRE(*row >= 0, "%s: Lmax + 1 - state_len = %d positions exceed the supported 4096", who, Lmax + 1 - state_len);
    return 0;
}

inline int dense_check(const char* who, int state_len, int N, int T, int layout_5s) {
    BH_REQUIRE(state_len >= 1 && state_len <= 5, "%s: state_len must be in 1..5 (got %d)", who, state_len);
    BH_REQUIRE(N > 0 && T > 0, "%s: empty problem N=%d T=%d", who, N, T);
    BH_REQUIRE(layout_5s == 0 || layout_5s == 1, "%s: layout_5s must be 0 or 1 (got %d)", who, layout_5s);
    return 0;
}

}  // namespace bh
