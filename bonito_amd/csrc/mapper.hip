// The read mapper's device half ("Mapper"; the definition is tests/mapper_ref.py): minimizer sketching, seeding
// against a sorted index and the chaining DP. Base-level alignment of the chained span is bh_nw_align (nw.hip); sorting and the
// prefix sums between the launches are the caller's (torch.sort / torch.cumsum).
//
// Sketch: one workgroup per tile of 512 window ends of one sequence. The codes of the tile and of the w + k - 1 positions in front of
// it go to LDS, every thread computes the key of one k-mer (two where the halo needs them), every thread scans one window of at most
// 64 keys in LDS for its leftmost minimum, and a window end whose selection differs from its left neighbour's emits a minimizer (the
// selections never move left, so this emits every selected position once, in order). Ordered compaction: flags -> ballot / block scan
// -> tile counts -> one scan over the tiles -> the same kernel again, writing.
// Seed: one thread per query minimizer, binary search among the index's distinct keys; counted, then (after the caller's prefix sum)
// written as one sortable 64-bit word per anchor: read << 53 | strand << 52 | reference position << 21 | query position.
// Chain: one wave per read, four reads per workgroup. The anchors come in 64 at a time, one per lane, coalesced; the current anchor is
// broadcast with v_readlane, lane s scores the predecessor whose index is congruent to s modulo 64 - its coordinates and f stay in
// that lane's registers, which are the ring - and a wave-wide max over (score << 32 | index) picks the winner, the largest index among
// equal scores. f and the predecessor of 64 anchors are stored together. The wave then follows the predecessors from the best anchor,
// and one more pass over its anchors gives s2.
#include "kernels.h"
#include "pair_align.h"

namespace bh {

constexpr int SK_TILE = 512;                // window ends per workgroup = threads per workgroup
constexpr int MAP_MAX_W = 64, MAP_MIN_K = 11, MAP_MAX_K = 28;
constexpr int MAP_QBITS = 21, MAP_RBITS = 31;                 // anchor word: query position, reference position, strand, read
constexpr int MAP_MAX_READS = 1 << 10;
constexpr unsigned long long MAP_NONE = ~0ull;

__device__ __forceinline__ unsigned long long map_mix(unsigned long long x, unsigned long long mask) {
    x = (~x + (x << 21)) & mask;
    x = x ^ (x >> 24);
    x = (x + (x << 3) + (x << 8)) & mask;
    x = x ^ (x >> 14);
    x = (x + (x << 2) + (x << 4)) & mask;
    x = x ^ (x >> 28);
    x = (x + (x << 31)) & mask;
    return x;
}

struct SketchArgs {
    const int8_t* codes; long stride;
    const int* len; const int* tile_start;    // device: [n], [n + 1]
    int n, k, w;
    int* tile_count; const int* tile_off;
    long long* keys; int* pos; int8_t* strand; long capacity;
};

template <bool FILL>
__global__ __launch_bounds__(SK_TILE) void map_sketch_kernel(SketchArgs a) {
    __shared__ int8_t s_code[SK_TILE + MAP_MAX_W + MAP_MAX_K];           // positions p0 - w - k + 1 ...
    __shared__ unsigned long long s_key[SK_TILE + MAP_MAX_W];            // positions p0 - w ...: key << 1 | strand, or MAP_NONE
    __shared__ int s_sel[SK_TILE + 1];                                   // window ends p0 - 1 ...
    __shared__ int s_wave[SK_TILE / WAVE];
    const int b = blockIdx.x, tid = threadIdx.x, k = a.k, w = a.w;
    int lo = 0, hi = a.n;                                                // the last sequence whose first tile is not behind b
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.tile_start[mid] <= b) lo = mid; else hi = mid;
    }
    const int seq = lo, L = a.len[seq];
    const int p0 = (b - a.tile_start[seq]) * SK_TILE;
    const int8_t* codes = a.codes + (long)seq * a.stride;
    const int c0 = p0 - w - k + 1;
    for (int x = tid; x < SK_TILE + w + k - 1; x += SK_TILE) {
        const int p = c0 + x;
        s_code[x] = p >= 0 && p < L ? codes[p] : (int8_t)0;
    }
    __syncthreads();
    const unsigned long long mask = (1ull << (2 * k)) - 1;
    for (int x = tid; x < SK_TILE + w; x += SK_TILE) {                   // the k-mer that ends at p0 - w + x starts at s_code[x]
        unsigned long long fw = 0, rv = 0;
        bool bad = false;
        for (int t = 0; t < k; ++t) {
            const int c = s_code[x + t];
            bad |= c < 1 || c > 4;                                       // padding in front of and behind the sequence included
            const unsigned long long v = (unsigned long long)((c - 1) & 3);
            fw |= v << (2 * (k - 1 - t));
            rv |= (3ull - v) << (2 * t);
        }
        const unsigned long long kf = map_mix(fw, mask), kr = map_mix(rv, mask);
        s_key[x] = bad || kf == kr ? MAP_NONE : ((kf < kr ? kf : kr) << 1) | (kr < kf ? 1ull : 0ull);
    }
    __syncthreads();
    const int first_end = min(k + w - 2, L - 1);
    for (int x = tid; x < SK_TILE + 1; x += SK_TILE) {
        const int e = p0 - 1 + x;
        int arg = -1;
        if (e <= L - 1 && e >= k - 1 && e >= first_end) {
            unsigned long long best = MAP_NONE >> 1;
            for (int p = max(k - 1, e - w + 1); p <= e; ++p) {
                const unsigned long long v = s_key[p - p0 + w] >> 1;
                if (v < best) { best = v; arg = p; }                     // strictly: the leftmost of equal keys stays
            }
        }
        s_sel[x] = arg;
    }
    __syncthreads();
    const int sel = s_sel[tid + 1];
    const bool flag = sel >= 0 && sel != s_sel[tid];
    const unsigned long long ballot = __ballot(flag);
    const int lane = tid & (WAVE - 1), wv = tid / WAVE;
    const int rank = __popcll(ballot & ((1ull << lane) - 1));
    if (lane == 0) s_wave[wv] = __popcll(ballot);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < SK_TILE / WAVE; ++i) {
        const int c = s_wave[i];
        before += i < wv ? c : 0;
        total += c;
    }
    if constexpr (!FILL) {
        if (tid == 0) a.tile_count[b] = total;
    } else {
        const long o = (long)a.tile_off[b] + before + rank;
        if (flag && o < a.capacity) {
            const unsigned long long v = s_key[sel - p0 + w];
            a.keys[o] = (long long)(v >> 1);
            a.pos[o] = sel;
            a.strand[o] = (int8_t)(v & 1);
        }
    }
}

constexpr int SCAN_THREADS = 1024;

// One workgroup: off[0 .. m] = the exclusive prefix sums of count[0 .. m), then seq_off[s] = off[tile_start[s]] for s = 0 .. n.
__global__ __launch_bounds__(SCAN_THREADS) void map_scan_kernel(const int* count, int m, int* off, const int* tile_start, int n, int* seq_off) {
    __shared__ int s_sum[SCAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (m + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = min(m, tid * per), hi = min(m, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += count[i];
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {                          // inclusive scan of the per-thread sums
        const int v = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int run = s_sum[tid] - sum;
    for (int i = lo; i < hi; ++i) { off[i] = run; run += count[i]; }
    if (tid == SCAN_THREADS - 1) off[m] = s_sum[tid];
    __threadfence();
    __syncthreads();                                                     // the offsets are read back by other threads of this workgroup
    for (int s = tid; s <= n; s += SCAN_THREADS) seq_off[s] = __hip_atomic_load(off + tile_start[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SeedArgs {
    const long long* qkeys; const int* qpos; const int8_t* qstrand; const int* q_off; const int* q_len; int n; long n_min;
    const long long* ukeys; const int* ustart; const int* ucount; long n_ukeys; const int* rpos; const int8_t* rstrand;
    int k, max_occ;
    int* counts; const long long* offsets; long long* anchors; long capacity;
};

template <bool FILL>
__global__ __launch_bounds__(256) void map_seed_kernel(SeedArgs a) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.n_min) return;
    const long long key = a.qkeys[q];
    long lo = 0, hi = a.n_ukeys;                                         // the first distinct key that is not smaller
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (a.ukeys[mid] < key) lo = mid + 1; else hi = mid;
    }
    int cnt = 0;
    if (lo < a.n_ukeys && a.ukeys[lo] == key) cnt = a.ucount[lo];
    if (cnt > a.max_occ) cnt = 0;
    if constexpr (!FILL) {
        a.counts[q] = cnt;
    } else {
        if (cnt == 0) return;
        int rl = 0, rh = a.n;                                            // the read this minimizer belongs to
        while (rh - rl > 1) {
            const int mid = (rl + rh) >> 1;
            if (a.q_off[mid] <= q) rl = mid; else rh = mid;
        }
        const int qp = a.qpos[q], qs = a.qstrand[q], start = a.ustart[lo];
        const long long o = a.offsets[q];
        for (int j = 0; j < cnt; ++j) {
            if (o + j >= a.capacity) break;
            const int st = qs ^ a.rstrand[start + j];
            const int qq = st ? a.q_len[rl] - qp + a.k - 2 : qp;
            a.anchors[o + j] = ((long long)rl << (MAP_QBITS + MAP_RBITS + 1)) | ((long long)st << (MAP_QBITS + MAP_RBITS))
                               | ((long long)a.rpos[start + j] << MAP_QBITS) | (long long)qq;
        }
    }
}

struct ChainArgs {
    const long long* anchors; const int* contig; const int* off; int n;
    int k, max_dist, bandwidth;
    int* f; int* p; int* chain; int* result;
};

__device__ __forceinline__ int map_q(long long a) { return (int)(a & ((1ll << MAP_QBITS) - 1)); }
__device__ __forceinline__ int map_r(long long a) { return (int)((a >> MAP_QBITS) & ((1ll << MAP_RBITS) - 1)); }
__device__ __forceinline__ int map_group(long long a) { return (int)(a >> (MAP_QBITS + MAP_RBITS)); }      // read and strand

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, WAVE), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, WAVE);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void map_chain_kernel(ChainArgs a) {
    const int read = (int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE), lane = threadIdx.x & (WAVE - 1);
    if (read >= a.n) return;                                             // whole waves leave together
    const int a0 = a.off[read], cnt = a.off[read + 1] - a0;
    int* res = a.result + (long)read * 4;
    if (cnt <= 0) {
        if (lane == 0) { res[0] = 0; res[1] = 0; res[2] = 0; res[3] = -1; }
        return;
    }
    const long long* an = a.anchors + a0;
    const int* ctg = a.contig + a0;
    const int k = a.k;
    long long rk = 0;                                                    // the ring: this lane's anchor, its contig, its f
    int rc = -1, rf = 0;
    int best_f = 0, best_i = -1;
    for (int c0 = 0; c0 < cnt; c0 += WAVE) {
        const int il = c0 + lane;
        const long long ck = il < cnt ? an[il] : 0;
        const int cc = il < cnt ? ctg[il] : -1;
        int myp = -1;
        const int kend = min(WAVE, cnt - c0);
        for (int t = 0; t < kend; ++t) {
            const long long cur = ((long long)__builtin_amdgcn_readlane((int)(ck >> 32), t) << 32)
                                  | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)ck, t);
            const int curc = __builtin_amdgcn_readlane(cc, t);
            const int j = lane < t ? c0 + lane : c0 - WAVE + lane;       // the anchor this lane's registers hold
            unsigned long long packed = 0;
            if (j >= 0 && map_group(rk) == map_group(cur) && rc == curc) {
                const int dr = map_r(cur) - map_r(rk), dq = map_q(cur) - map_q(rk);
                const int g = dr > dq ? dr - dq : dq - dr;
                if (dq > 0 && dq <= a.max_dist && dr > 0 && dr <= a.max_dist && g <= a.bandwidth) {
                    const int cost = g == 0 ? 0 : ((5 * g) >> 5) + ((31 - __clz(g)) >> 1);
                    const int sc = rf + min(min(dq, dr), k) - cost;
                    if (sc > k) packed = ((unsigned long long)(unsigned)sc << 32) | (unsigned)j;
                }
            }
            packed = wave_max_u64(packed);
            const int fi = packed ? (int)(packed >> 32) : k;
            const int pi = packed ? (int)(unsigned)packed : -1;
            if (fi > best_f) { best_f = fi; best_i = c0 + t; }           // the smallest index among equals
            if (lane == t) { rk = ck; rc = cc; rf = fi; myp = pi; }
        }
        if (il < cnt) { a.f[a0 + il] = rf; a.p[a0 + il] = myp; }
    }
    __threadfence();                                                     // f and p are read back below, by other lanes of this wave
    int len = 0, first = best_i;
    for (int i = best_i; i >= 0 && len < cnt;) {                         // every lane walks (the loads are one address); lane 0 writes
        if (lane == 0) a.chain[a0 + len] = i;
        ++len;
        first = i;
        const int prev = __hip_atomic_load(a.p + a0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        i = prev < i ? prev : -1;                                        // a predecessor always has a smaller index
    }
    const long long ek = an[best_i];
    const int eg = map_group(ek), ec = ctg[best_i], r_lo = map_r(an[first]), r_hi = map_r(ek);
    int s2 = 0;
    for (int x = lane; x < cnt; x += WAVE) {
        const long long v = an[x];
        const int r = map_r(v);
        if (map_group(v) != eg || ctg[x] != ec || r < r_lo || r > r_hi)
            s2 = max(s2, __hip_atomic_load(a.f + a0 + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) s2 = max(s2, __shfl_xor(s2, d, WAVE));
    if (lane == 0) { res[0] = len; res[1] = best_f; res[2] = s2; res[3] = best_i; }
}

// ---- end extension (the definition is tests/mapper_ext_ref.py) ---------------------------------------------------------------------
// One wave per end, four ends per workgroup. The band |j - i| <= 32 is marched over anti-diagonals a = i + j: the cells of one
// anti-diagonal all have the parity of a, so at most 33 of the 65 diagonals are live in a step and lane t holds the diagonal
// d = 2 t - 32 + (a & 1). The diagonal predecessor (i-1, j-1) is this lane's value two steps back; (i-1, j) is the diagonal d + 1 and
// (i, j-1) the diagonal d - 1 of the step before: one of them is this lane's own previous value, the other its neighbour's (lane
// t + 1 on odd steps, lane t - 1 on even ones), one __shfl per step. Cells outside the matrix or the band hold EXT_NEG exactly, so
// a predecessor that does not exist never wins. The two traceback bits of a cell go to LDS (8 rows x 2 parities per word, one word
// column per lane, 8.6 KB per wave); the walk back and the run-length encoding follow in the same kernel.
constexpr int EXT_MAX = 512, EXT_BAND = 32, EXT_LANES = EXT_BAND + 1;
constexpr int EXT_TB_WORDS = (EXT_MAX / 8 + 1) * EXT_LANES;
constexpr int EXT_NEG = -(1 << 28), EXT_BIAS = 1 << 20;
constexpr int EXT_MATCH = 2, EXT_PENALTY = 4;

struct ExtArgs {
    const int8_t* reads; long stride; const int* read_len; int n_reads;
    const int8_t* ref; long ref_len;
    const int* ends; int n_ends;
    int* result; unsigned* runs; int runs_cap;
};

struct ExtLds {
    unsigned tb[EXT_TB_WORDS];               // [row >> 3][lane]: 4 bits per row, the even anti-diagonal's cell in the low two
    int8_t q[EXT_MAX];                       // the query tail, nearest base first: 1..4, 0 = no base
    int8_t r[EXT_MAX + EXT_BAND];            // the reference tail: 1..4, 5 = no base (never equal to a query code that is none)
};

__device__ __forceinline__ void ext_wave_sync() {                        // LDS written by other lanes of this wave is read behind this
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void map_extend_kernel(ExtArgs a) {
    __shared__ ExtLds s_all[4];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    const int e = blockIdx.x * 4 + wave;
    if (e >= a.n_ends) return;                                           // whole waves leave together; there is no workgroup barrier
    ExtLds& s = s_all[wave];
    const int* en = a.ends + (long)e * 6;
    const int row = en[0], strand = en[1], side = en[2], qp = en[3];
    const long rp = en[4], lim = en[5];
    int* res = a.result + (long)e * 4;
    unsigned* out = a.runs + (long)e * a.runs_cap;
    bool ok = row >= 0 && row < a.n_reads && (strand == 0 || strand == 1) && (side == 0 || side == 1) && rp >= 0 && rp <= a.ref_len
              && lim >= 0 && lim <= a.ref_len && (side ? lim >= rp : lim <= rp);
    const int len = ok ? a.read_len[row] : 0;
    ok = ok && len >= 0 && len <= a.stride && qp >= 0 && qp <= len;
    if (!ok) {                                                           // an end that does not fit its read or the reference: nothing is read
        if (lane == 0) { res[0] = 0; res[1] = 0; res[2] = 0; res[3] = -1; }
        return;
    }
    const int m = min(side ? len - qp : qp, EXT_MAX);
    const int n = (int)min(side ? lim - rp : rp - lim, (long)(m + EXT_BAND));
    if (m == 0 || n == 0) {                                              // every cell but (0,0) is negative
        if (lane == 0) { res[0] = 0; res[1] = 0; res[2] = 0; res[3] = 0; }
        return;
    }
    const int8_t* rd = a.reads + (long)row * a.stride;
    for (int x = lane; x < m; x += WAVE) {
        const int p = side ? qp + x : qp - 1 - x;                        // position on the aligned strand
        int c = strand ? rd[len - 1 - p] : rd[p];
        c = c >= 1 && c <= 4 ? (strand ? 5 - c : c) : 0;
        s.q[x] = (int8_t)c;
    }
    for (int x = lane; x < n; x += WAVE) {
        const int c = a.ref[side ? rp + x : rp - 1 - x];
        s.r[x] = (int8_t)(c >= 1 && c <= 4 ? c : 5);
    }
    ext_wave_sync();
    const int t = lane;
    int prev1 = t == EXT_BAND / 2 ? 0 : EXT_NEG;                         // a = 0: the cell (0,0) on the diagonal 0
    int prev2 = EXT_NEG;
    int best_s = 0, best_i = 0, best_j = 0;                              // (0,0); a lane meets its cells in the order of i + j
    for (int ad = 1; ad <= m + n; ++ad) {
        const int p = ad & 1;
        const int d = 2 * t - EXT_BAND + p;
        const int nb = __shfl(prev1, (p ? t + 1 : t - 1) & (WAVE - 1), WAVE);
        const int up = p ? nb : prev1;                                   // (i-1, j)
        const int left = p ? prev1 : (t == 0 ? EXT_NEG : nb);            // (i, j-1)
        const int i = (ad - d) >> 1, j = (ad + d) >> 1;
        int v = EXT_NEG;
        if (t <= EXT_BAND - p && i >= 0 && j >= 0 && i <= m && j <= n) {
            unsigned dir = 0;
            if (i >= 1 && j >= 1) v = prev2 + (s.q[i - 1] == s.r[j - 1] ? EXT_MATCH : -EXT_PENALTY);
            if (up - EXT_PENALTY > v) { v = up - EXT_PENALTY; dir = 1; }
            if (left - EXT_PENALTY > v) { v = left - EXT_PENALTY; dir = 2; }
            unsigned* w = &s.tb[(i >> 3) * EXT_LANES + t];
            const int sh = (i & 7) * 4 + p * 2;
            *w = (*w & ~(3u << sh)) | (dir << sh);
            if (v > best_s) { best_s = v; best_i = i; best_j = j; }
        }
        prev2 = prev1;
        prev1 = v;
    }
    // (S + 2^20) << 32 | (65535 - (i + j)) << 16 | (65535 - i): every field is non-negative and fits its width (0 <= S + 2^20 < 2^21,
    // i + j <= 1056, i <= 512), so the larger word has the larger S, among equal S the smaller i + j, among those the smaller i
    unsigned long long key = ((unsigned long long)(unsigned)(best_s + EXT_BIAS) << 32) | ((unsigned)(0xFFFF - (best_i + best_j)) << 16)
                             | (unsigned)(0xFFFF - best_i);
    key = wave_max_u64(key);
    const int score = (int)(key >> 32) - EXT_BIAS;
    const int ei = 0xFFFF - (int)(key & 0xFFFF), ej = 0xFFFF - (int)((key >> 16) & 0xFFFF) - ei;
    ext_wave_sync();
    // every lane walks (the LDS reads are one address); lane 0 writes. The first walk counts the runs, the second stores them: in walk
    // order at the left end (the reversed tails run towards the span), in the opposite order at the right end
    int n_runs = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int i = ei, j = ej, k = 0, cur = -1, cnt = 0;
        while (i > 0 || j > 0) {
            const int dd = min(max(j - i + EXT_BAND, 0), 2 * EXT_BAND);   // a path never leaves the band; the index stays inside anyway
            const unsigned dir = (s.tb[(i >> 3) * EXT_LANES + (dd >> 1)] >> ((i & 7) * 4 + (dd & 1) * 2)) & 3u;
            int op;
            if (dir == 0 && i > 0 && j > 0) { op = s.q[i - 1] == s.r[j - 1] ? 0 : 1; --i; --j; }
            else if ((dir == 1 && i > 0) || j == 0) { op = 2; --i; }
            else { op = 3; --j; }
            if (op == cur) { ++cnt; continue; }
            if (cur >= 0) {
                if (pass && lane == 0) out[side ? n_runs - 1 - k : k] = ((unsigned)cnt << 2) | (unsigned)cur;
                ++k;
            }
            cur = op;
            cnt = 1;
        }
        if (cur >= 0) {
            if (pass && lane == 0) out[side ? n_runs - 1 - k : k] = ((unsigned)cnt << 2) | (unsigned)cur;
            ++k;
        }
        n_runs = k;
    }
    if (lane == 0) { res[0] = score; res[1] = ei; res[2] = ej; res[3] = n_runs; }
}

struct SketchLayout { size_t len, tile_start, tile_count, tile_off, total; };

static long sketch_tiles(int len) { return len > 0 ? ((long)len + SK_TILE - 1) / SK_TILE : 0; }

static void sketch_layout(int n, long tiles, SketchLayout* L) {
    const auto up = align_up256;
    L->len = 0;
    L->tile_start = up((size_t)n * sizeof(int));
    L->tile_count = L->tile_start + up(((size_t)n + 1) * sizeof(int));
    L->tile_off = L->tile_count + up((size_t)(tiles + 1) * sizeof(int));
    L->total = L->tile_off + up((size_t)(tiles + 1) * sizeof(int));
}

}  // namespace bh

int bh_k_map_sketch_tile() { return bh::SK_TILE; }

size_t bh_k_map_sketch_workspace(int n, long total_len) {
    if (n <= 0 || total_len < 0 || total_len >= (1l << 31)) return 0;
    bh::SketchLayout L;
    bh::sketch_layout(n, total_len / bh::SK_TILE + n, &L);
    return L.total;
}

int bh_k_map_sketch(const void* codes, long stride, const int* lengths, int n, int k, int w, void* workspace, size_t workspace_bytes,
                    long long* keys, int* pos, int8_t* strand, long capacity, int* offsets, hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(n > 0, "map_sketch: n must be positive (got %d)", n);
    BH_REQUIRE(codes && lengths && workspace && keys && pos && strand && offsets, "map_sketch: null pointer");
    BH_REQUIRE(k >= MAP_MIN_K && k <= MAP_MAX_K, "map_sketch: k must be in %d..%d (got %d)", MAP_MIN_K, MAP_MAX_K, k);
    BH_REQUIRE(w >= 1 && w <= MAP_MAX_W, "map_sketch: w must be in 1..%d (got %d)", MAP_MAX_W, w);
    BH_REQUIRE(stride >= 0 && capacity >= 0, "map_sketch: negative stride or capacity");
    long total = 0, need = 0, tiles = 0;
    std::vector<int> head(2 * (size_t)n + 1);
    for (int i = 0; i < n; ++i) {
        const int len = lengths[i];
        BH_REQUIRE(len >= 0, "map_sketch: sequence %d has a negative length (%d)", i, len);
        BH_REQUIRE(n == 1 || len <= stride, "map_sketch: sequence %d: length %d exceeds the row stride %ld", i, len, stride);
        head[i] = len;
        head[n + i] = (int)tiles;
        total += len;
        need += len >= k ? len - k + 1 : 0;
        tiles += sketch_tiles(len);
        BH_REQUIRE(total < (1l << 31), "map_sketch: the sequences of one call must total fewer than 2^31 bases");
    }
    head[2 * (size_t)n] = (int)tiles;
    BH_REQUIRE(capacity >= need, "map_sketch: the output holds %ld minimizers, %ld may be needed (one per k-mer)", capacity, need);
    SketchLayout L;
    sketch_layout(n, tiles, &L);
    BH_REQUIRE(workspace_bytes >= L.total, "map_sketch: workspace of %zu bytes, %zu needed (bh_map_sketch_workspace(%d, %ld))",
               workspace_bytes, L.total, n, total);
    char* ws = (char*)workspace;
    // the lengths are a host array (just validated): they and the first tile of every sequence go to the head of the workspace
    BH_CHECK_HIP(hipMemcpyWithStream(ws + L.len, head.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
    BH_CHECK_HIP(hipMemcpyWithStream(ws + L.tile_start, head.data() + n, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
    SketchArgs a{(const int8_t*)codes, stride, (const int*)(ws + L.len), (const int*)(ws + L.tile_start), n, k, w,
                 (int*)(ws + L.tile_count), (const int*)(ws + L.tile_off), keys, pos, strand, capacity};
    if (tiles) {
        hipLaunchKernelGGL(map_sketch_kernel<false>, dim3((unsigned)tiles), dim3(SK_TILE), 0, stream, a);
        BH_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, a.tile_count, (int)tiles, (int*)(ws + L.tile_off),
                       a.tile_start, n, offsets);
    BH_CHECK_HIP(hipGetLastError());
    if (tiles) {
        hipLaunchKernelGGL(map_sketch_kernel<true>, dim3((unsigned)tiles), dim3(SK_TILE), 0, stream, a);
        BH_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

int bh_k_map_seed(const long long* qkeys, const int* qpos, const int8_t* qstrand, const int* q_offsets, const int* q_lengths, int n,
                  long n_min, const long long* ukeys, const int* ustart, const int* ucount, long n_ukeys, const int* rpos,
                  const int8_t* rstrand, int k, int max_occ, int* counts, const long long* offsets, long long* anchors, long capacity,
                  hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(n > 0 && n <= MAP_MAX_READS, "map_seed: n must be in 1..%d (got %d)", MAP_MAX_READS, n);
    BH_REQUIRE(n_min >= 0 && n_ukeys >= 0 && capacity >= 0, "map_seed: negative count");
    BH_REQUIRE(k >= MAP_MIN_K && k <= MAP_MAX_K, "map_seed: k must be in %d..%d (got %d)", MAP_MIN_K, MAP_MAX_K, k);
    BH_REQUIRE(max_occ >= 1, "map_seed: max_occ must be positive (got %d)", max_occ);
    BH_REQUIRE(q_offsets && q_lengths && counts, "map_seed: null pointer");
    BH_REQUIRE(!offsets || anchors, "map_seed: offsets without an anchor buffer");
    if (n_min == 0) return 0;
    BH_REQUIRE(qkeys && qpos && qstrand, "map_seed: null pointer");
    BH_REQUIRE(n_ukeys == 0 || (ukeys && ustart && ucount && rpos && rstrand), "map_seed: null pointer");
    SeedArgs a{qkeys, qpos, qstrand, q_offsets, q_lengths, n, n_min, ukeys, ustart, ucount, n_ukeys, rpos, rstrand, k, max_occ,
               counts, offsets, anchors, capacity};
    const unsigned blocks = (unsigned)((n_min + 255) / 256);
    if (offsets) hipLaunchKernelGGL(map_seed_kernel<true>, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(map_seed_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

int bh_k_map_chain(const long long* anchors, const int* contigs, const int* offsets, int n, long n_anchors, int k, int max_dist,
                   int bandwidth, int* f, int* p, int* chain, int* result, hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(n > 0 && n <= MAP_MAX_READS, "map_chain: n must be in 1..%d (got %d)", MAP_MAX_READS, n);
    BH_REQUIRE(n_anchors >= 0 && n_anchors < (1l << 31), "map_chain: the anchors of one call must number fewer than 2^31 (got %ld)", n_anchors);
    BH_REQUIRE(k >= MAP_MIN_K && k <= MAP_MAX_K, "map_chain: k must be in %d..%d (got %d)", MAP_MIN_K, MAP_MAX_K, k);
    BH_REQUIRE(max_dist >= 1 && bandwidth >= 0, "map_chain: max_dist must be positive and bandwidth not negative");
    BH_REQUIRE(offsets && result, "map_chain: null pointer");
    BH_REQUIRE(n_anchors == 0 || (anchors && contigs && f && p && chain), "map_chain: null pointer");
    ChainArgs a{anchors, contigs, offsets, n, k, max_dist, bandwidth, f, p, chain, result};
    hipLaunchKernelGGL(map_chain_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

int bh_k_map_extend_max() { return bh::EXT_MAX; }
int bh_k_map_extend_band() { return bh::EXT_BAND; }

int bh_k_map_extend(const int8_t* reads, long stride, const int* read_len, int n_reads, const int8_t* ref, long ref_len, const int* ends,
                    int n_ends, int* result, unsigned* runs, int runs_cap, hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(n_ends >= 0, "map_extend: n_ends must not be negative (got %d)", n_ends);
    BH_REQUIRE(runs_cap >= 2 * EXT_MAX + EXT_BAND, "map_extend: runs_cap must be at least %d (got %d)", 2 * EXT_MAX + EXT_BAND, runs_cap);
    BH_REQUIRE(n_reads >= 0 && stride >= 0 && ref_len >= 0 && ref_len < (1l << 31), "map_extend: negative count, stride or reference length, or a reference of 2^31 bases or more");
    if (n_ends == 0) return 0;
    BH_REQUIRE(reads && read_len && ref && ends && result && runs, "map_extend: null pointer");
    ExtArgs a{reads, stride, read_len, n_reads, ref, ref_len, ends, n_ends, result, runs, runs_cap};
    hipLaunchKernelGGL(map_extend_kernel, dim3((unsigned)((n_ends + 3) / 4)), dim3(256), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
