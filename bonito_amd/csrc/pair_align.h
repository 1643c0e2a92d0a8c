// What the two pairwise aligners share: align.hip (Smith-Waterman and its semi-global mode) and nw.hip (banded global alignment).
// Each piece is written ONCE here and the kernels and entry points of the two files are written in terms of them.
//
// Device code: rows per lane and per pass, the DPP wave shift, the hand-off of a pass's last row, the address of a traceback word and
// the run-length writer of the tracebacks. Host code: the argument checks with the walk over the pairs, the copy of the lengths and
// the two launches. The cell recurrences, the band window, the end cell, the result rows and the workspace layouts stay in their files.
#pragma once
#include <type_traits>
#include <vector>

#include "common.h"

namespace bh {

constexpr int PA_R = 8;                     // query rows per lane
constexpr int PA_ROWS = WAVE * PA_R;        // query rows per pass

// what both argument structs begin with
struct PairArgs {
    const int8_t* seq; long seq_stride;
    const int8_t* ref; long ref_stride;
    const int* seq_len; const int* ref_len;   // the caller's host arrays while checked, then device copies at the head of the workspace
    int* result; unsigned* ops; long ops_stride; int* n_ops;
};

// value of the lane below (lane - 1); lane 0, which has no source, keeps `first`
__device__ __forceinline__ int wave_shr1(int first, int v) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// The hand-off of a pass's last row to the next pass, N values per column. Lane 63 finishes window column t - 63 at step t; lane
// (column & 63) keeps its outgoing values in a register, and after 64 columns, or at the `last` column of the window, the wave stores
// them coalesced into the boundary row (indexed by window column: the caller adds the window's first column).
template <int N>
struct PassHandoff {
    typedef typename std::conditional<N == 1, int, int2>::type Cell;
    int v[N] = {};
    __device__ __forceinline__ void step(int t, int last, int lane, const int (&out)[N], Cell* row) {
        const int c = t - (WAVE - 1);
        if (c >= 0) {
            if (lane == (c & (WAVE - 1))) {
#pragma unroll
                for (int x = 0; x < N; ++x) v[x] = __builtin_amdgcn_readlane(out[x], WAVE - 1);
            }
            if ((c & (WAVE - 1)) == WAVE - 1 || c == last) {
                const int col = (c & ~(WAVE - 1)) + lane;
                if (col <= c) {
                    if constexpr (N == 1) row[col] = v[0];
                    else row[col] = make_int2(v[0], v[1]);
                }
            }
        }
    }
};

// Traceback words of a pair are stored as [pass][step][lane]: the lane that owns `row` (8 rows a lane) works on window column `col` at
// step col + lane, and the `bits` bits of its 8 cells make one word, so a wave's store of a step is contiguous. -> the word's index
// and the shift of the row's bits in it
struct TraceAt { size_t word; int shift; };
__device__ __forceinline__ TraceAt trace_at(int pass, int steps, int col, int row, int bits) {
    const int ln = (row & (PA_ROWS - 1)) >> 3;
    return {((size_t)pass * steps + col + ln) * WAVE + ln, bits * (row & 7)};
}

// The run-length writer of a traceback. ops: 0 '=', 1 'X', 2 'I', 3 'D'; a run is (length << 2) | op. The walk emits last to first;
// finish() closes the open run, turns the stored runs round and returns their number (which may exceed the capacity: the host checks it)
struct RunWriter {
    unsigned* ops; long cap;
    int cnt[4] = {0, 0, 0, 0};
    int run_op = -1, run_len = 0, nruns = 0;
    __device__ __forceinline__ RunWriter(unsigned* ops_, long cap_) : ops(ops_), cap(cap_) {}
    __device__ __forceinline__ void flush() {
        if (run_len) {
            if (ops && nruns < cap) ops[nruns] = ((unsigned)run_len << 2) | (unsigned)run_op;
            ++nruns;
        }
    }
    __device__ __forceinline__ void emit(int op, int len = 1) {
        cnt[0] += op == 0 ? len : 0; cnt[1] += op == 1 ? len : 0; cnt[2] += op == 2 ? len : 0; cnt[3] += op == 3 ? len : 0;
        if (op == run_op) { run_len += len; return; }
        flush();
        run_op = op; run_len = len;
    }
    __device__ __forceinline__ int finish() {
        flush();
        if (ops) {
            const int w = nruns < cap ? nruns : (int)cap;
            for (int x = 0, y = w - 1; x < y; ++x, --y) { const unsigned v = ops[x]; ops[x] = ops[y]; ops[y] = v; }
        }
        return nruns;
    }
};

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// The checks every entry makes, and the walk over the pairs (a.seq_len / a.ref_len: the caller's host arrays). need(m, r) -> the most
// CIGAR runs a pair of these lengths can have; it is called once per pair, after the pair's lengths passed.
template <class Need>
static int pair_batch_begin(const char* who, int max_len, const PairArgs& a, int n, const void* workspace, int* max_seq, int* max_ref,
                            Need need_of) {
    BH_REQUIRE(n > 0, "%s_align: n must be positive (got %d)", who, n);
    BH_REQUIRE(a.seq && a.ref && a.seq_len && a.ref_len && workspace && a.result, "%s_align: null pointer", who);
    BH_REQUIRE(a.seq_stride >= 0 && a.ref_stride >= 0 && a.ops_stride >= 0, "%s_align: negative stride", who);
    BH_REQUIRE(!a.n_ops || a.ops, "%s_align: n_ops without an ops buffer", who);
    *max_seq = *max_ref = 0;
    for (int i = 0; i < n; ++i) {
        const int m = a.seq_len[i], r = a.ref_len[i];
        BH_REQUIRE(m >= 0 && r >= 0, "%s_align: pair %d has a negative length (%d, %d)", who, i, m, r);
        BH_REQUIRE(m <= a.seq_stride && r <= a.ref_stride, "%s_align: pair %d: lengths (%d, %d) exceed the row strides (%ld, %ld)", who, i, m,
                   r, a.seq_stride, a.ref_stride);
        BH_REQUIRE(m <= max_len && r <= max_len, "%s_align: pair %d: lengths (%d, %d) exceed the supported %d", who, i, m, r, max_len);
        const long need = need_of(m, r);
        BH_REQUIRE(!a.ops || need <= a.ops_stride, "%s_align: pair %d may need %ld CIGAR runs, the ops rows hold %ld", who, i, need,
                   a.ops_stride);
        *max_seq = m > *max_seq ? m : *max_seq;
        *max_ref = r > *max_ref ? r : *max_ref;
    }
    return 0;
}

// the lengths are host arrays (they were just validated): one blocking copy to the head of the workspace, ordered on the stream;
// a.seq_len / a.ref_len then name the device copies
static int pair_lengths_to_device(PairArgs* a, int n, void* workspace, hipStream_t stream) {
    std::vector<int> lens(a->seq_len, a->seq_len + n);
    lens.insert(lens.end(), a->ref_len, a->ref_len + n);
    BH_CHECK_HIP(hipMemcpyWithStream(workspace, lens.data(), lens.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    a->seq_len = (const int*)workspace;
    a->ref_len = (const int*)workspace + n;
    return 0;
}

// the forward kernel, one wave per pair, then the traceback kernel, one pair per thread
template <class Args>
static int pair_launch(void (*forward)(Args), void (*traceback)(Args, int), const Args& a, int n, hipStream_t stream) {
    hipLaunchKernelGGL(forward, dim3(n), dim3(WAVE), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(traceback, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, a, n);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace bh
