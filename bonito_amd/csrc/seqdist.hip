// CTC-CRF sequence likelihood and forced alignment on gfx950: the two scans the reference takes from closed koi.ctc
// (`logZ_cu`, `viterbi_alignments`; reference bonito/crf/model.py:126-143) behind CTC_CRF.ctc_loss / ctc_viterbi_alignments.
//
// The chain (exactly CTC_CRF.prepare_ctc_scores, crf/model.py:110-124): a target row holds labels 1..4 (0 = padding), len of them;
// targets0 = max(targets - 1, 0); with k = state_len the chain has n = len + 1 - k positions, position j = the k-mer
// targets0[j .. j + k) (oldest base most significant). Per time step position j has
//     a stay edge:             5S layout scores[5 kmer_j],                         4S (koi) layout the scalar blank_score
//     a move edge j-1 -> j:    5S layout scores[5 kmer_j + 1 + targets0[j-1]],     4S layout scores[4 kmer_j + targets0[j-1]]
// and the kernel gathers both from the score row itself: no [T][N][L] stay / move tensor exists anywhere.
//
// Log scan (bh_crf_seq_logz):   alpha_0 = [0, -inf, ...];  alpha_{t+1}[j] = logaddexp(alpha_t[j] + stay_t[j], alpha_t[j-1] + move_t[j]);
//     result alpha_T[n-1] in fp32 (the reference scans `scores.to(torch.float32)`); -inf where n - 1 > T.
// Max scan (bh_crf_seq_viterbi): the same with max; a cell remembers ONE BIT, "entered by the move edge", set only when the move
//     candidate is strictly greater: TIES RESOLVE TO STAY. Traceback from position n-1 gives align[t] = the position occupied after
//     step t (non-decreasing, steps of at most 1, align[T-1] = n-1, the position before step 0 is 0), and best = the path score.
//     A chunk with n - 1 > T has no alignment: best = -inf and align = -1 throughout. What koi's viterbi_alignments returns is not
//     known (koi is closed and the reference never calls ctc_viterbi_alignments): this compact form is this project's own definition.
// Free start (bh_crf_seq_logz_free, koi layout only): ln of the sum over every alignment AND every start state of a path that emits
//     exactly the sequence - the numerator of ln P(sequence | scores) (oracle_seq_logprob_f64). The fixed-start chain above pins the
//     first k-mer; here the first k emissions pass through states whose leading digits are still those of the unknown start state.
//     seq_prefix_kernel scans these dense levels 1 .. k-1 (4^(k-i) states at level i; level 0 is t * blank_score in closed form) and
//     writes, per step, the mass that enters chain position 0 (the k-mer of the first k bases); the chain kernel then starts from
//     alpha_0 = -inf everywhere and adds that term to position 0 each step. Sequences shorter than k end inside the dense levels and
//     are finished by the prefix kernel alone.
// Dense Log scan (bh_crf_logz_dense): CTC_CRF.logZ in fp32 for either layout with strides - what ctc_loss(normalise_scores=True)
//     needs for the reference's [T][N][5S] tensor (bh_crf_logz serves the contiguous koi layout).
//
// Kernel shape: a latency chain. Thread `tid` of a chunk owns the P consecutive positions tid P .. tid P + P - 1 in registers; the only
// value that crosses threads is the neighbour's last alpha. Up to 512 positions a chunk is ONE WAVE (P = 1, 2, 4, 8) and that value
// comes by a wave shift - no LDS, no barrier; up to 4096 positions it is four waves (P = 4, 8, 16) with one LDS hand-off and one barrier
// per step. The gathered edge scores of the next SU steps sit in a register ring, so the chain never waits on memory. The traceback
// bits leave as one 64-bit ballot per wave and position slot: exactly one bit per cell, [N][T][waves * P] words of workspace.
//
// Supported range (checked, never truncated): 1 <= state_len <= 5, 1 <= T, Lmax + 1 - state_len <= 4096, labels 0..4.
// target_lengths live on the device, so a chunk whose length is below state_len (fixed start) or above Lmax yields NaN; the Python
// surface rejects both before anything is launched.
//
// lse2 / lse_n, the label read, the chain pieces (problem description, gather offsets, ring load, hand-off, Log-scan step), the
// dense pieces and the (threads, positions per thread) instance list are in seq_chain.h, which seqdist_grad.hip builds on as well.
#include <math.h>

#include "common.h"
#include "kernels.h"
#include "seq_chain.h"

namespace bh {

constexpr int SU = 4;            // prefetch depth (time steps)
constexpr int STB = 64;          // traceback block (time steps)

struct SeqArgs {
    ChainArgs c;
    unsigned long long* bits;    // [N][T][waves * P] (Max scan)
    const float* inject;         // [N][T] (free start) or null
    float* out;                  // [N]
    int* align;                  // [N][T] (Max scan)
};

template <int P, bool MULTI, bool VIT>
__global__ __launch_bounds__(256) void seq_scan_kernel(SeqArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ChainArgs& c = p.c;
    const int n = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, T = c.T;
    const int len = c.lens[n];
    const int npos = len + 1 - c.k;
    const bool free_start = p.inject != nullptr;
    if (len > c.Lmax || (npos <= 0 && !free_start)) {                       // argument error on the device: NaN, never a truncated answer
        if (tid == 0) p.out[n] = __builtin_nanf("");
        if (VIT)
            for (int t = tid; t < T; t += NT) p.align[(long)n * T + t] = -1;
        return;
    }
    if (npos <= 0) return;                                                  // free start, shorter than k: seq_prefix_kernel wrote the result

    // ---- the chain: gather offsets of this thread's positions ----
    int so[P], mo[P];
#pragma unroll
    for (int i = 0; i < P; ++i) chain_offsets(c, n, tid * P + i, so[i], mo[i]);
    const half_t* sc = c.scores + (long)n * c.s_n;
    const float* inj = free_start ? p.inject + (long)n * T : nullptr;

    float sv[SU][P], mv[SU][P], iv[SU];
    auto load = [&](int slot, int t) {
        const int tt = min(t, T - 1);                                       // (rows beyond the end are never used)
        chain_load(c, sc + (long)tt * c.s_t, so, mo, sv[slot], mv[slot]);
        iv[slot] = free_start ? inj[tt] : -INFINITY;
    };

    float a[P];
#pragma unroll
    for (int i = 0; i < P; ++i) a[i] = -INFINITY;
    if (tid == 0 && !free_start) a[0] = 0.0f;

    float* edge = (float*)smem;                                             // [2][NT] (MULTI)
    int cb = 0;
    const int WP = (NT / WAVE) * P;
    unsigned long long* bits = VIT ? p.bits + (long)n * T * WP : nullptr;

#pragma unroll
    for (int u = 0; u < SU; ++u) load(u, u);
    for (int t0 = 0; t0 < T; t0 += SU) {
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const int t = t0 + u;
            if (t < T) {                                                    // uniform across the workgroup
                const float prev = chain_from_left<MULTI>(a[P - 1], edge, cb, tid, NT);
                if constexpr (!VIT) {
                    chain_log_step(a, prev, sv[u], mv[u]);
                    if (free_start && tid == 0) a[0] = lse2(a[0], iv[u]);
                } else {
                    unsigned moved = 0;
#pragma unroll
                    for (int i = P - 1; i >= 0; --i) {                      // descending: position i reads the OLD alpha of i - 1
                        const float in = (i ? a[i - 1] : prev) + mv[u][i];
                        const float st = a[i] + sv[u][i];
                        const bool m = in > st;                             // ties: stay
                        a[i] = m ? in : st;
                        moved |= (unsigned)m << i;
                    }
                    const int lane = tid & 63, w = tid >> 6;
                    unsigned long long mine = 0;
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        const unsigned long long m = __ballot((moved >> i) & 1);
                        if (lane == i) mine = m;
                    }
                    if (lane < P) bits[(long)t * WP + w * P + lane] = mine;
                }
                load(u, t + SU);
            }
        }
    }

    // ---- result: alpha_T[npos - 1] ----
    const int last = npos - 1;
    if (last / P == tid) {
        float r = a[0];
#pragma unroll
        for (int i = 1; i < P; ++i)
            if (last % P == i) r = a[i];
        p.out[n] = r;
    }
    if constexpr (VIT) {
        int* al = p.align + (long)n * T;
        if (last > T) {                                                     // no alignment exists (best = -inf was written above)
            for (int t = tid; t < T; t += NT) al[t] = -1;
            return;
        }
        __threadfence();   // the traceback bits of this workgroup -> visible to its own later loads
        __syncthreads();
        // ---- traceback in LDS-staged blocks of STB steps: all threads copy, the first thread chases ----
        unsigned long long* stage = (unsigned long long*)(smem + 2 * NT * sizeof(float));   // [STB][WP]
        int* res = (int*)(stage + STB * WP);                                                // [STB]
        int* s_pos = res + STB;
        if (tid == 0) *s_pos = last;
        for (int thi = T; thi > 0; thi -= STB) {
            const int tlo = max(0, thi - STB);
            const int nw = (thi - tlo) * WP;
            for (int e = tid; e < nw; e += NT) stage[e] = bits[(long)tlo * WP + e];
            __syncthreads();
            if (tid == 0) {
                int pos = *s_pos;
                for (int t = thi - 1; t >= tlo; --t) {
                    res[t - tlo] = pos;
                    const int g = pos / P;
                    const unsigned long long word = stage[(t - tlo) * WP + (g >> 6) * P + pos % P];
                    pos -= (int)((word >> (g & 63)) & 1);
                }
                *s_pos = pos;
            }
            __syncthreads();
            for (int e = tid; e < thi - tlo; e += NT) al[tlo + e] = res[e];
            __syncthreads();
        }
    }
}

// ---- free start: the dense levels 1 .. k-1 of the first k emissions, and the mass entering chain position 0 (level k) -------------
struct PrefixArgs {
    SeqArgs s;
    float* inject;               // [N][T]
    int total;                   // states of levels 1 .. k
};

__global__ __launch_bounds__(384) void seq_prefix_kernel(PrefixArgs q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ChainArgs& p = q.s.c;
    float* D = (float*)smem;                                                // [2][total]
    const int n = blockIdx.x, x = threadIdx.x, k = p.k;
    const int len = p.lens[n];
    if (len > p.Lmax) return;                                               // (the chain kernel reports it)
    // level i = 1 .. k holds 4^(k-i) states u; state (i, u) is the k-mer u 4^i + (first i bases), level k = chain position 0
    int lvl = 0, u = 0, off = 0, off_prev = 0;
    {
        int o = 0;
        for (int i = 1; i <= k; ++i) {
            const int cnt = 1 << (2 * (k - i));
            if (x >= o && x < o + cnt) { lvl = i; u = x - o; off = o; off_prev = o - 4 * cnt; }
            o += cnt;
        }
    }
    const bool active = lvl != 0;
    int s2 = 0;
    if (active) {
        int pre = 0;
        for (int d = 0; d < lvl; ++d) pre = pre * 4 + target0(p, n, d);
        s2 = (u << (2 * lvl)) + pre;
    }
    const int cnt = 1 << (2 * (k - lvl));                                   // states of this level = stride between the four predecessors
    const half_t* sc = p.scores + (long)n * p.s_n + 4 * s2;
    float* inj = q.inject + (long)n * p.T;

    for (int i = x; i < 2 * q.total; i += blockDim.x) D[i] = -INFINITY;
    __syncthreads();

    float ring[SU][4];
    auto load = [&](int slot, int t) {
        const half_t* row = sc + (long)min(t, p.T - 1) * p.s_t;
#pragma unroll
        for (int r = 0; r < 4; ++r) ring[slot][r] = active ? (float)row[r] : 0.0f;
    };
    int cb = 0;
#pragma unroll
    for (int v = 0; v < SU; ++v) load(v, v);
    for (int t0 = 0; t0 < p.T; t0 += SU) {
#pragma unroll
        for (int v = 0; v < SU; ++v) {
            const int t = t0 + v;
            if (t < p.T) {                                                  // uniform across the workgroup
                const float* d = D + cb * q.total;
                if (active) {
                    float c[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pa = lvl == 1 ? (float)t * p.blank : d[off_prev + r * cnt + u];
                        c[r] = pa + ring[v][r];
                    }
                    const float in = lse_n<true>(c);
                    if (lvl < k) D[(cb ^ 1) * q.total + off + u] = lse2(d[off + u] + p.blank, in);
                    else inj[t] = in;
                }
                cb ^= 1;
                __syncthreads();
                load(v, t + SU);
            }
        }
    }
    if (x == 0 && len < k) {                                                // the sequence ends inside the dense levels
        float r;
        if (len <= 0) {
            r = (float)p.T * p.blank + __logf((float)(1 << (2 * k)));
        } else {
            const float* d = D + cb * q.total;
            int o = 0;
            for (int i = 1; i < len; ++i) o += 1 << (2 * (k - i));
            const int c = 1 << (2 * (k - len));
            float m = -INFINITY;
            for (int i = 0; i < c; ++i) m = fmaxf(m, d[o + i]);
            r = m;
            if (m != -INFINITY) {
                float sum = 0.0f;
                for (int i = 0; i < c; ++i) sum += __expf(d[o + i] - m);
                r = m + __logf(sum);
            }
        }
        q.s.out[n] = r;
    }
}

// ---- CTC_CRF.logZ in fp32, both layouts, strided: one thread per state, alpha ping-pongs in LDS ------------------------------------
struct DenseArgs {
    const half_t* scores;
    int N, T, S, five;
    float blank;
    long s_n, s_t;
    float* out;
};

__global__ __launch_bounds__(1024) void crf_dense_logz_kernel(DenseArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* al = (float*)smem;                                               // [2][S]
    const int n = blockIdx.x, j = threadIdx.x, S = p.S, q = S >> 2;
    const bool active = j < S;
    const half_t* sc = p.scores + (long)n * p.s_n + (p.five ? 5 : 4) * (active ? j : 0);
    if (active) al[j] = 0.0f;
    __syncthreads();
    float ring[SU][5];
    auto load = [&](int slot, int t) { dense_load(p, sc + (long)min(t, p.T - 1) * p.s_t, ring[slot]); };
    int cb = 0;
#pragma unroll
    for (int v = 0; v < SU; ++v) load(v, v);
    for (int t0 = 0; t0 < p.T; t0 += SU) {
#pragma unroll
        for (int v = 0; v < SU; ++v) {
            if (t0 + v < p.T) {                                             // uniform across the workgroup
                if (active) al[(cb ^ 1) * S + j] = dense_step(al + cb * S, j, q, ring[v]);
                cb ^= 1;
                __syncthreads();
                load(v, t0 + v + SU);
            }
        }
    }
    if (j == 0) p.out[n] = dense_final(al + cb * S, S);
}

// the chain kernels of the instance list, in its order
typedef void (*SeqKernel)(SeqArgs);
struct SeqKernels { SeqKernel max, log; };
#define BH_SEQ_ROW(NT, P, MULTI) {seq_scan_kernel<P, MULTI, true>, seq_scan_kernel<P, MULTI, false>},
static const SeqKernels kSeqKernels[] = {BH_SEQ_INSTANCES(BH_SEQ_ROW)};
#undef BH_SEQ_ROW

}  // namespace bh

size_t bh_k_crf_seq_workspace(int N, int T, int Lmax, int state_len) {
    if (N <= 0 || T <= 0 || Lmax < 0 || state_len < 1 || state_len > 5) return 0;
    const int row = bh::chain_instance(Lmax, state_len);
    if (row < 0) return 0;
    const int threads = bh::kSeqGeometry[row].threads, per = bh::kSeqGeometry[row].per;
    const size_t bits = (size_t)N * T * (threads / 64) * per * sizeof(unsigned long long);
    const size_t inj = (size_t)N * T * sizeof(float);
    return (bits > inj ? bits : inj) + 512;
}

// mode 0: Log scan, 1: Max scan with traceback, 2: Log scan with a free start (koi layout)
int bh_k_crf_seq(const void* scores, int N, int T, int state_len, int layout_5s, float blank, long s_n, long s_t,
                 const void* targets, int target_bytes, int Lmax, const int* lens, void* workspace, float* out, int* align,
                 int mode, hipStream_t stream) {
    using namespace bh;
    if (int rc = chain_check("crf_seq", state_len, N, T, layout_5s, target_bytes, Lmax, mode == 2 ? 0 : state_len)) return rc;
    BH_REQUIRE(mode != 2 || !layout_5s, "crf_seq: the free-start sum is defined on the koi layout only");
    int row;
    if (int rc = chain_instance_check("crf_seq", Lmax, state_len, &row)) return rc;
    const int threads = kSeqGeometry[row].threads, P = kSeqGeometry[row].per;
    SeqArgs a{{(const half_t*)scores, N, T, state_len, layout_5s, blank, s_n, s_t, targets, target_bytes, Lmax, lens},
              (unsigned long long*)workspace, nullptr, out, align};
    if (mode == 2) {
        int total = 0;
        for (int i = 1; i <= state_len; ++i) total += 1 << (2 * (state_len - i));
        PrefixArgs q{a, (float*)workspace, total};
        const int th = (total + 63) / 64 * 64;
        hipLaunchKernelGGL(seq_prefix_kernel, dim3(N), dim3(th), (size_t)2 * total * sizeof(float), stream, q);
        BH_CHECK_HIP(hipGetLastError());
        a.inject = (const float*)workspace;
    }
    const bool vit = mode == 1;
    const size_t lds = 2 * threads * sizeof(float) + (vit ? (size_t)STB * (threads / 64) * P * 8 + STB * 4 + 16 : 0);
    hipLaunchKernelGGL(vit ? kSeqKernels[row].max : kSeqKernels[row].log, dim3(N), dim3(threads), lds, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

int bh_k_crf_logz_dense(const void* scores, int N, int T, int state_len, int layout_5s, float blank, long s_n, long s_t,
                        float* out, hipStream_t stream) {
    using namespace bh;
    if (int rc = dense_check("crf_logz_dense", state_len, N, T, layout_5s)) return rc;
    const int S = 1 << (2 * state_len);
    DenseArgs a{(const half_t*)scores, N, T, S, layout_5s, blank, s_n, s_t, out};
    hipLaunchKernelGGL(crf_dense_logz_kernel, dim3(N), dim3(S < 64 ? 64 : S), (size_t)2 * S * sizeof(float), stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
