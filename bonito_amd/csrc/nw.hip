// Batched banded global alignment under unit costs with a traceback ("Duplex"): the engine's counterpart of
// edlib.align(query, ref, task="path") behind the reference's basespace duplex caller (bonito/cli/duplex.py:224-269).
//
//   D(0,0) = 0, D(i,0) = i, D(0,j) = j
//   D(i,j) = min(D(i-1,j-1) + [q_i != r_j], D(i,j-1) + 1 (op D: consumes a ref base), D(i-1,j) + 1 (op I: consumes a query base))
//
// Band: with delta = n - m and half-width k only the cells whose diagonal j - i lies in [min(0, delta) - k, max(0, delta) + k] are
// computed; every other cell (the borders D(i,0) and D(0,j) among them) counts as +infinity. A banded distance d is accepted when
// floor((d - |delta|) / 2) <= k: then every optimal path, and every predecessor that ties on one, lies inside the band with its true
// value, and distance and traceback equal those of the full matrix. The caller runs a rejected pair again with k doubled.
//
// Forward kernel: one wave per pair, the layout of sw_forward_kernel (align.hip; pair_align.h). A pass covers 512 query rows, lane l owns 8
// consecutive rows, and the reference columns of the pass's band window [jlo, jhi) stream through the lanes one column per step; the
// bottom value of a strip and the reference base move to the next lane with one DPP wave shift each. Each cell leaves 2 traceback
// bits (the predecessor: diagonal first, then D, then I); the 8 cells of a lane and a step make 16 bits, stored as
// [pass][step][lane], so a wave's store is one contiguous 128 bytes. Traceback memory is passes * (window + 63) * 128 bytes with
// window <= 511 + band width: proportional to m * band, never m * n. Offsets into it are 64-bit.
// Traceback kernel: one pair per thread applies the acceptance test, walks the bits back from (m, n) and writes the run-length ops.
#include "kernels.h"
#include "pair_align.h"

namespace bh {

constexpr int NW_MAX_LEN = 65536;
constexpr int NW_MAX_K = 65536;             // at this half-width the band holds the whole matrix of the longest pair
constexpr int NW_INF = 1 << 29;             // "+infinity": INF plus one step per cell of the longest path stays below 2^31

struct NwArgs : PairArgs {
    int k;
    unsigned short* trace; size_t trace_stride;   // 16-bit words per pair
    int pass_steps;                           // steps reserved per pass: min(max_ref, 511 + band width) + 63
    int* bound; size_t bound_stride;          // [pair][2][bound_stride]: the last row of a pass by absolute column, ping-pong by parity
    int* dist;                                // [pair]
};

__global__ __launch_bounds__(WAVE) void nw_forward_kernel(NwArgs a) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int m = a.seq_len[pair], n = a.ref_len[pair];
    if (m == 0 || n == 0) return;                                            // the traceback kernel writes the single run
    const int8_t* seq = a.seq + (long)pair * a.seq_stride;
    const int8_t* ref = a.ref + (long)pair * a.ref_stride;
    const int delta = n - m;
    const int lo = min(0, delta) - a.k, hi = max(0, delta) + a.k;            // the band's diagonals j - i
    const int passes = (m + PA_ROWS - 1) / PA_ROWS;
    int jhi_prev = 0, dist = NW_INF;
    for (int p = 0; p < passes; ++p) {
        const int base = p * PA_ROWS, row0 = base + lane * PA_R;
        const int jlo = max(0, base + lo);                                   // window of the pass: columns (0-based) [jlo, jhi)
        const int jhi = min((long)n, (long)min(m, base + PA_ROWS) + hi);
        const int W = jhi - jlo, S = W + WAVE - 1;
        int q[PA_R], H[PA_R];
#pragma unroll
        for (int r = 0; r < PA_R; ++r) {
            q[r] = row0 + r < m ? (int)seq[row0 + r] : 0;
            // the cell to the left of the window: the border D(i, 0) = i where the window starts at column 0 and the border is
            // inside the band, otherwise outside the band
            H[r] = jlo == 0 && row0 + r + 1 <= -lo ? row0 + r + 1 : NW_INF;
        }
        const int* bin = a.bound + ((size_t)pair * 2 + (p & 1)) * a.bound_stride;
        int* bout = a.bound + ((size_t)pair * 2 + ((p + 1) & 1)) * a.bound_stride;
        int hdiag = jlo == 0 ? (row0 <= -lo ? row0 : NW_INF) : (lane == 0 ? bin[jlo - 1] : NW_INF);
        int h_out = NW_INF, c_out = 0;
        const bool keep = p + 1 < passes;                                    // the next pass needs this pass's last row
        // the lane's word of step 0 (where it would work on column -lane); a step on is WAVE words on
        unsigned short* tr = a.trace + (size_t)pair * a.trace_stride + trace_at(p, a.pass_steps, -lane, row0, 2).word;
        PassHandoff<1> hand;
        for (int t0 = 0; t0 < S; t0 += WAVE) {
            const int cj = t0 + lane, ja = jlo + cj;
            const int cchunk = cj < W ? (int)ref[ja] : 0;
            int hchunk = NW_INF;                                             // the row above the pass: D(base, ja + 1)
            if (cj < W) {
                if (p == 0) hchunk = ja + 1 <= hi ? ja + 1 : NW_INF;
                else if (ja < jhi_prev) hchunk = bin[ja];
            }
            const int kend = min(WAVE, S - t0);
            for (int k = 0; k < kend; ++k) {
                const int t = t0 + k;
                const int hup = wave_shr1(__builtin_amdgcn_readlane(hchunk, k), h_out);
                const int refc = wave_shr1(__builtin_amdgcn_readlane(cchunk, k), c_out);
                c_out = refc;
                const int u = t - lane;
                if (u >= 0 && u < W) {
                    const int dg = jlo + u - row0;                           // diagonal of the lane's first row at this column
                    int hd = hdiag, hu = hup;
                    hdiag = hup;
                    unsigned bits = 0;
#pragma unroll
                    for (int r = 0; r < PA_R; ++r) {
                        const int sub = hd + (q[r] != refc ? 1 : 0), del = H[r] + 1, ins = hu + 1;
                        int h = min(sub, min(del, ins));
                        // the diagonal first, then D, then I
                        const unsigned src = h == sub ? 0u : h == del ? 1u : 2u;
                        bits |= src << (2 * r);
                        h = (dg - r >= lo && dg - r <= hi) ? h : NW_INF;
                        hd = H[r]; H[r] = h; hu = h;
                    }
                    h_out = hu;
                    tr[(size_t)t * WAVE] = (unsigned short)bits;
                }
                if (keep) hand.step(t, W - 1, lane, {h_out}, bout + jlo);
            }
        }
        jhi_prev = jhi;
        if (!keep && ((m - 1 - base) >> 3) == lane) {                        // the last window ends at column n - 1: H is D(., n)
#pragma unroll
            for (int r = 0; r < PA_R; ++r)
                if (((m - 1) & (PA_R - 1)) == r) dist = H[r];
            a.dist[pair] = dist;
        }
    }
}

// result row: distance, counts of = X I D, runs, k, status
// (0 accepted, 1 the band was too narrow: only distance - an upper bound -, k and status are meaningful)
__global__ __launch_bounds__(WAVE) void nw_traceback_kernel(NwArgs a, int npairs) {
    const int pair = blockIdx.x * WAVE + threadIdx.x;
    if (pair >= npairs) return;
    const int m = a.seq_len[pair], n = a.ref_len[pair];
    int* res = a.result + (long)pair * 8;
    const int delta = n - m, ad = delta < 0 ? -delta : delta;
    const int d = m && n ? a.dist[pair] : m + n;
    if (m && n && (d - ad) / 2 > a.k) {
        res[0] = d; res[1] = 0; res[2] = 0; res[3] = 0; res[4] = 0; res[5] = 0; res[6] = a.k; res[7] = 1;
        if (a.n_ops) a.n_ops[pair] = 0;
        return;
    }
    const int8_t* seq = a.seq + (long)pair * a.seq_stride;
    const int8_t* ref = a.ref + (long)pair * a.ref_stride;
    const unsigned short* trace = a.trace + (size_t)pair * a.trace_stride;
    const int lo = min(0, delta) - a.k;
    RunWriter w(a.ops ? a.ops + (long)pair * a.ops_stride : nullptr, a.ops_stride);
    int i = m, j = n, status = 0;                                            // 1-based: the cell D(i, j)
    while (i > 0 && j > 0) {                                                 // every turn consumes a base: at most m + n turns
        const int p = (i - 1) / PA_ROWS;
        const int u = j - 1 - max(0, p * PA_ROWS + lo);
        if (u < 0 || u + WAVE - 1 >= a.pass_steps) { status = 3; break; }    // outside the stored window: cannot happen once accepted
        const TraceAt at = trace_at(p, a.pass_steps, u, i - 1, 2);
        const unsigned src = (trace[at.word] >> at.shift) & 3u;
        if (src == 0) { w.emit(seq[i - 1] == ref[j - 1] ? 0 : 1); --i; --j; }
        else if (src == 1) { w.emit(3); --j; }
        else { w.emit(2); --i; }
    }
    if (status == 0) {
        if (j > 0) w.emit(3, j);                                             // on row 0 only D remains
        if (i > 0) w.emit(2, i);                                             // on column 0 only I remains
    }
    const int nruns = w.finish();
    res[0] = d; res[1] = w.cnt[0]; res[2] = w.cnt[1]; res[3] = w.cnt[2]; res[4] = w.cnt[3]; res[5] = nruns; res[6] = a.k; res[7] = status;
    if (a.n_ops) a.n_ops[pair] = nruns;
}

struct NwLayout { size_t dist, bound, bound_stride, trace, trace_stride, total; int pass_steps; };

static bool nw_layout(int n, int max_seq, int max_ref, long max_band, NwLayout* L) {
    if (n <= 0 || max_seq < 0 || max_ref < 0 || max_seq > NW_MAX_LEN || max_ref > NW_MAX_LEN || max_band < 1) return false;
    const auto up = align_up256;
    const size_t passes = ((size_t)max_seq + PA_ROWS - 1) / PA_ROWS;
    const long window = max_band + PA_ROWS - 1 < max_ref ? max_band + PA_ROWS - 1 : max_ref;
    L->pass_steps = (int)window + WAVE - 1;
    L->dist = up((size_t)2 * n * sizeof(int));
    L->bound = L->dist + up((size_t)n * sizeof(int));
    L->bound_stride = passes > 1 ? ((size_t)max_ref + WAVE - 1) / WAVE * WAVE : 0;
    L->trace = L->bound + up((size_t)n * 2 * L->bound_stride * sizeof(int));
    L->trace_stride = max_ref ? passes * (size_t)L->pass_steps * WAVE : 0;
    L->total = L->trace + (size_t)n * L->trace_stride * sizeof(unsigned short);
    return true;
}

}  // namespace bh

size_t bh_k_nw_workspace(int n, int max_seq, int max_ref, long max_band) {
    bh::NwLayout L;
    return bh::nw_layout(n, max_seq, max_ref, max_band, &L) ? L.total : 0;
}

int bh_k_nw_align(const void* seqs, long seq_stride, const int* seq_lens, const void* refs, long ref_stride, const int* ref_lens,
                  int n, int k, void* workspace, size_t workspace_bytes, int* result, unsigned* ops, long ops_stride, int* n_ops,
                  hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(k >= 1 && k <= NW_MAX_K, "nw_align: the band half-width must be in 1..%d (got %d)", NW_MAX_K, k);
    PairArgs head{(const int8_t*)seqs, seq_stride, (const int8_t*)refs, ref_stride, seq_lens, ref_lens, result, ops, ops_stride, n_ops};
    int max_seq, max_ref;
    long max_band = 1;
    if (int rc = pair_batch_begin("nw", NW_MAX_LEN, head, n, workspace, &max_seq, &max_ref, [&](int m, int r) {
            const long band = (long)(m > r ? m - r : r - m) + 2L * k + 1;
            max_band = band > max_band ? band : max_band;
            return (long)m + r;                                              // every op consumes a base
        })) return rc;
    NwLayout L;
    BH_REQUIRE(nw_layout(n, max_seq, max_ref, max_band, &L), "nw_align: unsupported shape");
    BH_REQUIRE(workspace_bytes >= L.total, "nw_align: workspace of %zu bytes, %zu needed (bh_nw_workspace(%d, %d, %d, %ld))",
               workspace_bytes, L.total, n, max_seq, max_ref, max_band);
    if (int rc = pair_lengths_to_device(&head, n, workspace, stream)) return rc;
    char* ws = (char*)workspace;
    NwArgs a{head, k, (unsigned short*)(ws + L.trace), L.trace_stride, L.pass_steps, (int*)(ws + L.bound), L.bound_stride,
             (int*)(ws + L.dist)};
    return pair_launch(nw_forward_kernel, nw_traceback_kernel, a, n, stream);
}
