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
// Forward kernel: one wave per pair, the layout of sw_forward_kernel (align.hip). A pass covers 512 query rows, lane l owns 8
// consecutive rows, and the reference columns of the pass's band window [jlo, jhi) stream through the lanes one column per step; the
// bottom value of a strip and the reference base move to the next lane with one DPP wave shift each. Each cell leaves 2 traceback
// bits (the predecessor: diagonal first, then D, then I); the 8 cells of a lane and a step make 16 bits, stored as
// [pass][step][lane], so a wave's store is one contiguous 128 bytes. Traceback memory is passes * (window + 63) * 128 bytes with
// window <= 511 + band width: proportional to m * band, never m * n. Offsets into it are 64-bit.
// Traceback kernel: one pair per thread applies the acceptance test, walks the bits back from (m, n) and writes the run-length ops.
#include "common.h"
#include "kernels.h"
#include <vector>

namespace bh {

constexpr int NW_R = 8;                     // query rows per lane
constexpr int NW_ROWS = WAVE * NW_R;        // query rows per pass
constexpr int NW_MAX_LEN = 65536;
constexpr int NW_MAX_K = 65536;             // at this half-width the band holds the whole matrix of the longest pair
constexpr int NW_INF = 1 << 29;             // "+infinity": INF plus one step per cell of the longest path stays below 2^31

struct NwArgs {
    const int8_t* seq; long seq_stride;
    const int8_t* ref; long ref_stride;
    const int* seq_len; const int* ref_len;   // device copies at the head of the workspace
    int k;
    unsigned short* trace; size_t trace_stride;   // 16-bit words per pair
    int pass_steps;                           // steps reserved per pass: min(max_ref, 511 + band width) + 63
    int* bound; size_t bound_stride;          // [pair][2][bound_stride]: the last row of a pass by absolute column, ping-pong by parity
    int* dist;                                // [pair]
    int* result; unsigned* ops; long ops_stride; int* n_ops;
};

// value of the lane below (lane - 1); lane 0, which has no source, keeps `first`
__device__ __forceinline__ int nw_shr1(int first, int v) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

__global__ __launch_bounds__(WAVE) void nw_forward_kernel(NwArgs a) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int m = a.seq_len[pair], n = a.ref_len[pair];
    if (m == 0 || n == 0) return;                                            // the traceback kernel writes the single run
    const int8_t* seq = a.seq + (long)pair * a.seq_stride;
    const int8_t* ref = a.ref + (long)pair * a.ref_stride;
    const int delta = n - m;
    const int lo = min(0, delta) - a.k, hi = max(0, delta) + a.k;            // the band's diagonals j - i
    const int passes = (m + NW_ROWS - 1) / NW_ROWS;
    int jhi_prev = 0, dist = NW_INF;
    for (int p = 0; p < passes; ++p) {
        const int base = p * NW_ROWS, row0 = base + lane * NW_R;
        const int jlo = max(0, base + lo);                                   // window of the pass: columns (0-based) [jlo, jhi)
        const int jhi = min((long)n, (long)min(m, base + NW_ROWS) + hi);
        const int W = jhi - jlo, S = W + WAVE - 1;
        int q[NW_R], H[NW_R];
#pragma unroll
        for (int r = 0; r < NW_R; ++r) {
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
        unsigned short* tr = a.trace + (size_t)pair * a.trace_stride + (size_t)p * a.pass_steps * WAVE + lane;
        int oh = 0;
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
                const int hup = nw_shr1(__builtin_amdgcn_readlane(hchunk, k), h_out);
                const int refc = nw_shr1(__builtin_amdgcn_readlane(cchunk, k), c_out);
                c_out = refc;
                const int u = t - lane;
                if (u >= 0 && u < W) {
                    const int dg = jlo + u - row0;                           // diagonal of the lane's first row at this column
                    int hd = hdiag, hu = hup;
                    hdiag = hup;
                    unsigned bits = 0;
#pragma unroll
                    for (int r = 0; r < NW_R; ++r) {
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
                if (keep) {                                                  // lane 63 has just finished window column t - 63
                    const int c = t - (WAVE - 1);
                    if (c >= 0) {
                        if (lane == (c & (WAVE - 1))) oh = __builtin_amdgcn_readlane(h_out, WAVE - 1);
                        if ((c & (WAVE - 1)) == WAVE - 1 || c == W - 1) {
                            const int col = (c & ~(WAVE - 1)) + lane;
                            if (col <= c) bout[jlo + col] = oh;
                        }
                    }
                }
            }
        }
        jhi_prev = jhi;
        if (!keep && ((m - 1 - base) >> 3) == lane) {                        // the last window ends at column n - 1: H is D(., n)
#pragma unroll
            for (int r = 0; r < NW_R; ++r)
                if (((m - 1) & (NW_R - 1)) == r) dist = H[r];
            a.dist[pair] = dist;
        }
    }
}

// ops: 0 '=', 1 'X', 2 'I', 3 'D'; a run is (length << 2) | op. result row: distance, counts of = X I D, runs, k, status
// (0 accepted, 1 the band was too narrow: only distance - an upper bound -, k and status are meaningful)
__global__ __launch_bounds__(WAVE) void nw_traceback_kernel(NwArgs a, int npairs) {
    const int pair = blockIdx.x * WAVE + threadIdx.x;
    if (pair >= npairs) return;
    const int m = a.seq_len[pair], n = a.ref_len[pair];
    int* res = a.result + (long)pair * 8;
    unsigned* ops = a.ops ? a.ops + (long)pair * a.ops_stride : nullptr;
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
    int cnt[4] = {0, 0, 0, 0};
    int run_op = -1, run_len = 0, nruns = 0, status = 0;
    auto emit = [&](int op, int len) {
        cnt[0] += op == 0 ? len : 0; cnt[1] += op == 1 ? len : 0; cnt[2] += op == 2 ? len : 0; cnt[3] += op == 3 ? len : 0;
        if (op == run_op) { run_len += len; return; }
        if (run_len) {
            if (ops && nruns < a.ops_stride) ops[nruns] = ((unsigned)run_len << 2) | (unsigned)run_op;
            ++nruns;
        }
        run_op = op; run_len = len;
    };
    int i = m, j = n;                                                        // 1-based: the cell D(i, j)
    while (i > 0 && j > 0) {                                                 // every turn consumes a base: at most m + n turns
        const int p = (i - 1) / NW_ROWS, ln = ((i - 1) & (NW_ROWS - 1)) >> 3;
        const int u = j - 1 - max(0, p * NW_ROWS + lo);
        if (u < 0 || u + WAVE - 1 >= a.pass_steps) { status = 3; break; }    // outside the stored window: cannot happen once accepted
        const unsigned src = (trace[((size_t)p * a.pass_steps + u + ln) * WAVE + ln] >> (2 * ((i - 1) & 7))) & 3u;
        if (src == 0) { emit(seq[i - 1] == ref[j - 1] ? 0 : 1, 1); --i; --j; }
        else if (src == 1) { emit(3, 1); --j; }
        else { emit(2, 1); --i; }
    }
    if (status == 0) {
        if (j > 0) emit(3, j);                                               // on row 0 only D remains
        if (i > 0) emit(2, i);                                               // on column 0 only I remains
    }
    if (run_len) {
        if (ops && nruns < a.ops_stride) ops[nruns] = ((unsigned)run_len << 2) | (unsigned)run_op;
        ++nruns;
    }
    if (ops) {                                                               // the walk wrote the runs last to first
        const int w = nruns < a.ops_stride ? nruns : (int)a.ops_stride;
        for (int x = 0, y = w - 1; x < y; ++x, --y) { const unsigned v = ops[x]; ops[x] = ops[y]; ops[y] = v; }
    }
    res[0] = d; res[1] = cnt[0]; res[2] = cnt[1]; res[3] = cnt[2]; res[4] = cnt[3]; res[5] = nruns; res[6] = a.k; res[7] = status;
    if (a.n_ops) a.n_ops[pair] = nruns;
}

struct NwLayout { size_t dist, bound, bound_stride, trace, trace_stride, total; int pass_steps; };

static bool nw_layout(int n, int max_seq, int max_ref, long max_band, NwLayout* L) {
    if (n <= 0 || max_seq < 0 || max_ref < 0 || max_seq > NW_MAX_LEN || max_ref > NW_MAX_LEN || max_band < 1) return false;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t passes = ((size_t)max_seq + NW_ROWS - 1) / NW_ROWS;
    const long window = max_band + NW_ROWS - 1 < max_ref ? max_band + NW_ROWS - 1 : max_ref;
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
    BH_REQUIRE(n > 0, "nw_align: n must be positive (got %d)", n);
    BH_REQUIRE(seqs && refs && seq_lens && ref_lens && workspace && result, "nw_align: null pointer");
    BH_REQUIRE(k >= 1 && k <= NW_MAX_K, "nw_align: the band half-width must be in 1..%d (got %d)", NW_MAX_K, k);
    BH_REQUIRE(seq_stride >= 0 && ref_stride >= 0 && ops_stride >= 0, "nw_align: negative stride");
    BH_REQUIRE(!n_ops || ops, "nw_align: n_ops without an ops buffer");
    int max_seq = 0, max_ref = 0;
    long max_band = 1;
    for (int i = 0; i < n; ++i) {
        const int m = seq_lens[i], r = ref_lens[i];
        BH_REQUIRE(m >= 0 && r >= 0, "nw_align: pair %d has a negative length (%d, %d)", i, m, r);
        BH_REQUIRE(m <= seq_stride && r <= ref_stride, "nw_align: pair %d: lengths (%d, %d) exceed the row strides (%ld, %ld)", i, m, r,
                   seq_stride, ref_stride);
        BH_REQUIRE(m <= NW_MAX_LEN && r <= NW_MAX_LEN, "nw_align: pair %d: lengths (%d, %d) exceed the supported %d", i, m, r, NW_MAX_LEN);
        const long need = (long)m + r;                                       // every op consumes a base
        BH_REQUIRE(!ops || need <= ops_stride, "nw_align: pair %d may need %ld CIGAR runs, the ops rows hold %ld", i, need, ops_stride);
        const long band = (long)(m > r ? m - r : r - m) + 2L * k + 1;
        max_seq = m > max_seq ? m : max_seq;
        max_ref = r > max_ref ? r : max_ref;
        max_band = band > max_band ? band : max_band;
    }
    NwLayout L;
    BH_REQUIRE(nw_layout(n, max_seq, max_ref, max_band, &L), "nw_align: unsupported shape");
    BH_REQUIRE(workspace_bytes >= L.total, "nw_align: workspace of %zu bytes, %zu needed (bh_nw_workspace(%d, %d, %d, %ld))",
               workspace_bytes, L.total, n, max_seq, max_ref, max_band);
    char* ws = (char*)workspace;
    // the lengths are host arrays (they were just validated): one blocking copy to the head of the workspace, ordered on the stream
    std::vector<int> lens(seq_lens, seq_lens + n);
    lens.insert(lens.end(), ref_lens, ref_lens + n);
    BH_CHECK_HIP(hipMemcpyWithStream(ws, lens.data(), lens.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    NwArgs a{(const int8_t*)seqs, seq_stride, (const int8_t*)refs, ref_stride, (const int*)ws, (const int*)ws + n, k,
             (unsigned short*)(ws + L.trace), L.trace_stride, L.pass_steps, (int*)(ws + L.bound), L.bound_stride, (int*)(ws + L.dist),
             result, ops, ops_stride, n_ops};
    hipLaunchKernelGGL(nw_forward_kernel, dim3(n), dim3(WAVE), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(nw_traceback_kernel, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, a, n);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
