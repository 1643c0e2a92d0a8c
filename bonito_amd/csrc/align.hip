// Batched Smith-Waterman local alignment with affine gaps and a traceback ("Read accuracy"): the engine's
// counterpart of parasail.sw_trace_striped_32(seq, ref, open, extend, matrix) behind the reference's accuracy figures
// (bonito/cli/evaluate.py:37-67, bonito/util.py:346-368). Exact 32-bit integer scores.
//
//   E(i,j) = max(H(i,j-1) - open, E(i,j-1) - extend)        deletion  (consumes a ref base, CIGAR D)
//   F(i,j) = max(H(i-1,j) - open, F(i-1,j) - extend)        insertion (consumes a seq base, CIGAR I)
//   H(i,j) = max(0, H(i-1,j-1) + s(seq_i, ref_j), E(i,j), F(i,j))
//
// Forward kernel: one wave per pair. A pass covers 512 query rows: lane l owns the 8 consecutive rows [8l, 8l+8) of the pass
// and the reference streams through the lanes one column per step (lane l works on column t - l at step t). The bottom H and
// F of a strip and the reference base move to the next lane with one DPP wave shift each; lane 0 is fed from a register chunk
// (64 columns per coalesced load: the reference bases and, from the second pass on, the boundary row the previous pass left
// in the workspace). Each cell leaves 4 traceback bits (2: source of H, 1: E extended, 1: F extended); the 8 cells of a lane
// and a step make one dword, stored as [pass][step][lane] (trace_at, pair_align.h: the parts shared with nw.hip), so a wave's store is
// one contiguous 256 bytes.
// Traceback kernel: one pair per thread walks the bits back from the end cell, counts the ops and writes the run-length ops.
//
// Semi-global mode (template parameter SG; bh_sg_align, the counterpart of parasail.sg_trace_scan_32 behind the reference's duplex end
// repair, bonito/cli/duplex.py:240-243): H without the floor at 0, H(i,0) = H(0,j) = 0, the end cell is the largest H over the last row
// and the last column (the smallest i, then the smallest j), the walk stops on reaching row 0 or column 0, and the CIGAR covers both
// sequences completely - head and tail overhangs come out as one I or D run each.
#include "kernels.h"
#include "pair_align.h"

namespace bh {

constexpr int SW_MAX_LEN = 4096;
constexpr int SW_MAX_PARAM = 32767;         // |score parameter| bound: 4096 * 32767 < 2^31
constexpr int SW_NONE = -2147483647 - 1;     // semi-global: "no end cell yet", below every H
constexpr int SW_NEG = -(1 << 30);          // E / F "minus infinity": NEG - extend cannot wrap, and no H - open reaches it

struct SwArgs : PairArgs {
    int match, mismatch, open, ext;
    unsigned* trace; size_t trace_stride;     // dwords per pair
    int2* bound; size_t bound_stride;         // [pair][2][bound_stride] (H, F) of the last row of a pass, ping-pong by pass parity
    int* endcell;                             // [pair][4]: score, end_i, end_j
};

// SG: the semi-global mode (H without the floor at 0, the end cell on the last row or the last column)
template <bool SG>
__global__ __launch_bounds__(WAVE) void sw_forward_kernel(SwArgs a) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int m = a.seq_len[pair], n = a.ref_len[pair];
    int best = SG ? SW_NONE : 0, besti = -1, bestj = -1;
    if (m > 0 && n > 0) {
        const int8_t* seq = a.seq + (long)pair * a.seq_stride;
        const int8_t* ref = a.ref + (long)pair * a.ref_stride;
        const int S = n + WAVE - 1;                                          // steps of one pass
        const int passes = (m + PA_ROWS - 1) / PA_ROWS;
        const int match = a.match, mismatch = a.mismatch, open = a.open, ext = a.ext;
        for (int p = 0; p < passes; ++p) {
            const int row0 = p * PA_ROWS + lane * PA_R;
            int q[PA_R], H[PA_R], E[PA_R], bH[PA_R], bJ[PA_R];
#pragma unroll
            for (int r = 0; r < PA_R; ++r) {
                q[r] = row0 + r < m ? (int)seq[row0 + r] : 0;
                H[r] = 0; E[r] = SW_NEG; bH[r] = SG ? SW_NONE : 0; bJ[r] = 0;
            }
            int hdiag = 0, h_out = 0, f_out = SW_NEG, c_out = 0;
            const int2* bin = a.bound + ((size_t)pair * 2 + (p & 1)) * a.bound_stride;
            int2* bout = a.bound + ((size_t)pair * 2 + ((p + 1) & 1)) * a.bound_stride;
            const bool keep = p + 1 < passes;                                // the next pass needs this pass's last row
            // the lane's word of step 0 (where it would work on column -lane); a step on is WAVE words on
            unsigned* tr = a.trace + (size_t)pair * a.trace_stride + trace_at(p, S, -lane, row0, 4).word;
            PassHandoff<2> hand;
            for (int t0 = 0; t0 < S; t0 += WAVE) {
                const int cj = t0 + lane;
                const int cchunk = cj < n ? (int)ref[cj] : 0;
                int hchunk = 0, fchunk = SW_NEG;
                if (p > 0 && cj < n) { const int2 v = bin[cj]; hchunk = v.x; fchunk = v.y; }
                const int kend = min(WAVE, S - t0);
                for (int k = 0; k < kend; ++k) {
                    const int t = t0 + k;
                    const int hup = wave_shr1(__builtin_amdgcn_readlane(hchunk, k), h_out);
                    const int fup = wave_shr1(__builtin_amdgcn_readlane(fchunk, k), f_out);
                    const int refc = wave_shr1(__builtin_amdgcn_readlane(cchunk, k), c_out);
                    c_out = refc;
                    const int j = t - lane;
                    if (j >= 0 && j < n) {
                        int hd = hdiag, hu = hup, fu = fup;
                        hdiag = hup;
                        unsigned bits = 0;
#pragma unroll
                        for (int r = 0; r < PA_R; ++r) {
                            const int s = q[r] == refc ? match : mismatch;
                            const int eo = H[r] - open, ee = E[r] - ext;
                            const int fo = hu - open, fe = fu - ext;
                            const int e = max(eo, ee), f = max(fo, fe);
                            const int d = hd + s;
                            const int h = SG ? max(max(d, e), f) : max(max(max(d, e), f), 0);
                            // stop at H = 0 (local mode only), then the diagonal, then E, then F; E / F: the open wins a tie
                            const unsigned src = !SG && h == 0 ? 0u : h == d ? 1u : h == e ? 2u : 3u;
                            bits |= (src | (ee > eo ? 4u : 0u) | (fe > fo ? 8u : 0u)) << (4 * r);
                            // strict: the smallest j of a row; semi-global: only the last column and the last row can end
                            if ((!SG || j == n - 1 || row0 + r == m - 1) && h > bH[r]) { bH[r] = h; bJ[r] = j; }
                            hd = H[r]; H[r] = h; E[r] = e; hu = h; fu = f;
                        }
                        h_out = hu; f_out = fu;
                        tr[(size_t)t * WAVE] = bits;
                    }
                    if (keep) hand.step(t, n - 1, lane, {h_out, f_out}, bout);
                }
            }
#pragma unroll
            for (int r = 0; r < PA_R; ++r)                                   // ascending rows, strict: the smallest i of a lane
                if (row0 + r < m && bH[r] > best) { best = bH[r]; besti = row0 + r; bestj = bJ[r]; }
        }
    }
    // end cell: the largest H, among equals the smallest i, then the smallest j
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int ob = __shfl_xor(best, off), oi = __shfl_xor(besti, off), oj = __shfl_xor(bestj, off);
        if (ob > best || (ob == best && (oi < besti || (oi == besti && oj < bestj)))) { best = ob; besti = oi; bestj = oj; }
    }
    if (lane == 0) {
        a.endcell[pair * 4 + 0] = best;
        a.endcell[pair * 4 + 1] = besti;
        a.endcell[pair * 4 + 2] = bestj;
    }
}

// SG: the walk stops on reaching row 0 or column 0, and the CIGAR covers both sequences completely: what lies before the first and
// after the last aligned column comes out as one I or D run each (the counts include them)
template <bool SG>
__global__ __launch_bounds__(WAVE) void sw_traceback_kernel(SwArgs a, int npairs) {
    const int pair = blockIdx.x * WAVE + threadIdx.x;
    if (pair >= npairs) return;
    const int m = a.seq_len[pair], n = a.ref_len[pair];
    const int score = a.endcell[pair * 4 + 0], ei = a.endcell[pair * 4 + 1], ej = a.endcell[pair * 4 + 2];
    int* res = a.result + (long)pair * 10;
    if (SG && (m == 0 || n == 0)) {                                          // nothing to align: one run over the other sequence
        const int len = m + n;
        res[0] = 0; res[1] = 0; res[2] = 0; res[3] = m; res[4] = n; res[5] = 0; res[6] = -1; res[7] = 0; res[8] = -1; res[9] = len > 0;
        if (a.ops && len) a.ops[(long)pair * a.ops_stride] = ((unsigned)len << 2) | (m ? 2u : 3u);
        if (a.n_ops) a.n_ops[pair] = len > 0;
        return;
    }
    if ((!SG && score <= 0) || ei < 0 || ej < 0 || ei >= m || ej >= n) {
        res[0] = 0; res[1] = 0; res[2] = 0; res[3] = 0; res[4] = 0; res[5] = 0; res[6] = -1; res[7] = 0; res[8] = -1; res[9] = 0;
        if (a.n_ops) a.n_ops[pair] = 0;
        return;
    }
    const int8_t* seq = a.seq + (long)pair * a.seq_stride;
    const int8_t* ref = a.ref + (long)pair * a.ref_stride;
    const unsigned* trace = a.trace + (size_t)pair * a.trace_stride;
    RunWriter w(a.ops ? a.ops + (long)pair * a.ops_stride : nullptr, a.ops_stride);
    const int S = n + WAVE - 1;
    int i = ei, j = ej, state = 0;
    if (SG) {                                                                // the end cell lies on the last row or the last column
        if (n - 1 - ej > 0) w.emit(3, n - 1 - ej);
        if (m - 1 - ei > 0) w.emit(2, m - 1 - ei);
    }
    for (int it = 0; it < m + n && i >= 0 && j >= 0; ++it) {                // every turn consumes a base: at most m + n turns
        const TraceAt at = trace_at(i / PA_ROWS, S, j, i, 4);
        const unsigned bits = trace[at.word] >> at.shift;
        if (state == 0) {
            const unsigned src = bits & 3u;
            if (!SG && src == 0) break;
            if (src == 1) { w.emit(seq[i] == ref[j] ? 0 : 1); --i; --j; continue; }
            state = src == 2 ? 1 : 2;
        }
        if (state == 1) { w.emit(3); state = (bits & 4u) ? 1 : 0; --j; }
        else { w.emit(2); state = (bits & 8u) ? 2 : 0; --i; }
    }
    const int si = i, sj = j;                                                // one before the first aligned column
    if (SG) {
        if (si >= 0) w.emit(2, si + 1);
        if (sj >= 0) w.emit(3, sj + 1);
    }
    const int nruns = w.finish();
    res[0] = score; res[1] = w.cnt[0]; res[2] = w.cnt[1]; res[3] = w.cnt[2]; res[4] = w.cnt[3];
    res[5] = sj + 1; res[6] = ej; res[7] = si + 1; res[8] = ei; res[9] = nruns;
    if (a.n_ops) a.n_ops[pair] = nruns;
}

struct SwLayout { size_t endcell, bound, bound_stride, trace, trace_stride, total; };

static bool sw_layout(int n, int max_seq, int max_ref, SwLayout* L) {
    if (n <= 0 || max_seq < 0 || max_ref < 0 || max_seq > SW_MAX_LEN || max_ref > SW_MAX_LEN) return false;
    const auto up = align_up256;
    const size_t passes = ((size_t)max_seq + PA_ROWS - 1) / PA_ROWS;
    L->endcell = up((size_t)2 * n * sizeof(int));
    L->bound = L->endcell + up((size_t)4 * n * sizeof(int));
    L->bound_stride = passes > 1 ? ((size_t)max_ref + WAVE - 1) / WAVE * WAVE : 0;
    L->trace = L->bound + up((size_t)n * 2 * L->bound_stride * sizeof(int2));
    L->trace_stride = max_ref ? passes * ((size_t)max_ref + WAVE - 1) * WAVE : 0;
    L->total = L->trace + (size_t)n * L->trace_stride * sizeof(unsigned);
    return true;
}

}  // namespace bh

size_t bh_k_sw_workspace(int n, int max_seq, int max_ref) {
    bh::SwLayout L;
    return bh::sw_layout(n, max_seq, max_ref, &L) ? L.total : 0;
}

template <bool SG>
static int affine_align(const void* seqs, long seq_stride, const int* seq_lens, const void* refs, long ref_stride, const int* ref_lens,
                        int n, int match, int mismatch, int gap_open, int gap_extend, void* workspace, size_t workspace_bytes,
                        int* result, unsigned* ops, long ops_stride, int* n_ops, hipStream_t stream) {
    using namespace bh;
    const char* who = SG ? "sg" : "sw";
    BH_REQUIRE(match >= 1 && match <= SW_MAX_PARAM, "%s_align: match must be in 1..%d (got %d)", who, SW_MAX_PARAM, match);
    BH_REQUIRE(mismatch < match && mismatch >= -SW_MAX_PARAM, "%s_align: mismatch must be in %d..match-1 (got %d)", who, -SW_MAX_PARAM,
               mismatch);
    BH_REQUIRE(gap_extend >= 1, "%s_align: gap_extend must be at least 1 (got %d)", who, gap_extend);
    BH_REQUIRE(gap_open >= gap_extend && gap_open <= SW_MAX_PARAM, "%s_align: gap_open must be in gap_extend..%d (got open %d, extend %d)", who,
               SW_MAX_PARAM, gap_open, gap_extend);
    PairArgs head{(const int8_t*)seqs, seq_stride, (const int8_t*)refs, ref_stride, seq_lens, ref_lens, result, ops, ops_stride, n_ops};
    int max_seq, max_ref;
    // every op consumes a base, the first one two; the semi-global CIGAR may begin or end with an overhang run
    if (int rc = pair_batch_begin(who, SW_MAX_LEN, head, n, workspace, &max_seq, &max_ref,
                                  [](int m, int r) { return SG ? (long)m + r : m && r ? (long)m + r - 1 : 0; })) return rc;
    SwLayout L;
    BH_REQUIRE(sw_layout(n, max_seq, max_ref, &L), "%s_align: unsupported shape", who);
    BH_REQUIRE(workspace_bytes >= L.total, "%s_align: workspace of %zu bytes, %zu needed (bh_sw_workspace(%d, %d, %d))", who, workspace_bytes,
               L.total, n, max_seq, max_ref);
    if (int rc = pair_lengths_to_device(&head, n, workspace, stream)) return rc;
    char* ws = (char*)workspace;
    SwArgs a{head, match, mismatch, gap_open, gap_extend, (unsigned*)(ws + L.trace), L.trace_stride, (int2*)(ws + L.bound), L.bound_stride,
             (int*)(ws + L.endcell)};
    return pair_launch(sw_forward_kernel<SG>, sw_traceback_kernel<SG>, a, n, stream);
}

int bh_k_sw_align(const void* seqs, long seq_stride, const int* seq_lens, const void* refs, long ref_stride, const int* ref_lens,
                  int n, int match, int mismatch, int gap_open, int gap_extend, void* workspace, size_t workspace_bytes,
                  int* result, unsigned* ops, long ops_stride, int* n_ops, hipStream_t stream) {
    return affine_align<false>(seqs, seq_stride, seq_lens, refs, ref_stride, ref_lens, n, match, mismatch, gap_open, gap_extend,
                               workspace, workspace_bytes, result, ops, ops_stride, n_ops, stream);
}

int bh_k_sg_align(const void* seqs, long seq_stride, const int* seq_lens, const void* refs, long ref_stride, const int* ref_lens,
                  int n, int match, int mismatch, int gap_open, int gap_extend, void* workspace, size_t workspace_bytes,
                  int* result, unsigned* ops, long ops_stride, int* n_ops, hipStream_t stream) {
    return affine_align<true>(seqs, seq_stride, seq_lens, refs, ref_stride, ref_lens, n, match, mismatch, gap_open, gap_extend,
                              workspace, workspace_bytes, result, ops, ops_stride, n_ops, stream);
}
