// What training a QuartzNet CTC model (bonito.ctc) adds on gfx950: the backward of the depthwise convolution (bh_k_dwconv is its
// forward), the residual add with the block's activation and dropout, and the backward of the 1x1 decoder with its log-softmax
// (bh_k_ctc_head is its forward). The arithmetic is stated in include/bonito_hip.h under bh_dwconv1d_train_backward.
//
// Depthwise backward, x fp16 [N][L][C], dy fp16 [N][Lout][C], w fp32 [C][K], stride 1:
//   dx: a depthwise convolution of dy with the taps flipped. A workgroup owns 64 positions x 64 channels and keeps the dy rows with
//       their K - 1 halo and the weights (tap-major) in LDS; a thread owns 8 channels and every 32nd position, fmaf in tap order.
//   dw: a reduction over all N Lout rows for each of C K outputs. A workgroup owns a tile of 64 channels and a block of consecutive
//       units (a unit = 64 rows of one chunk; the block a function of the shape alone). Per unit it stages x with its halo and dy in LDS.
//       A thread owns one channel and KG consecutive taps (a wave = one tap group of the 64 channels, four groups cover K <= 4 KG), as
//       KG fp32 accumulators held over all its units: per 8 rows it reads a window of KG + 7 x values and 8 dy values from LDS for
//       8 KG fmaf, each accumulator in row order. The [block][C][K] planes go to the workspace and a second launch adds them in block
//       order (block_order_sum, train_common.h): no floating-point atomics, equal bytes from call to call.
// Residual + activation + dropout: one thread per 8 channels; keep is recomputed from (seed, stream_id, element index), never stored.
// Head backward: one thread per row recomputes the logits as ctc_head_kernel forms them, writes dx and dlogit (fp32 [M][8], workspace);
//   dw and db: a workgroup owns a block of rows (a function of M alone), a thread one feature column with 8 class accumulators in row
//   order; the bias column rides as feature F with x = 1; the blocks are added in block order.
// Every kernel of this file indexes with 64 bits.
#include <cmath>

#include "train_common.h"

namespace bh {
namespace {

// ---- depthwise convolution backward --------------------------------------------------------------------------------------------------------
constexpr int QD_T = 64;            // rows of a unit / positions of a dx tile
constexpr int QD_C = 64;            // channels of a tile
constexpr int QD_MAX_K = 127;
constexpr int QD_TB = 8;            // rows per window of the dw kernel
constexpr long QD_WORKGROUPS = 1024;

const char* qd_shape_error(int N, int L, int C, int K, int pad) {
    if (N < 1 || L < 1) return "N and L must be positive";
    if (C < 8 || C % 8 != 0) return "C must be a multiple of 8";
    if (K < 1 || K > QD_MAX_K) return "K must be in 1..127";
    if (pad < 0 || pad >= K) return "pad must be in 0..K-1";
    if ((long)L + 2 * pad - K + 1 < 1) return "the input is shorter than one window (Lout >= 1)";
    return nullptr;
}

// taps of a thread of the dw kernel: the smallest of 1, 2, 4, ... 32 with 4 KG >= K
inline int qd_tap_group(int K) {
    int kg = 1;
    while (4 * kg < K) kg *= 2;
    return kg;
}

struct QdLayout {
    int Lout, ctiles, tiles_t;
    long units, blocks, per_block;     // units = N tiles_t; a block = per_block consecutive units
    size_t part, total;                // part: fp32 [blocks][C][K]
    QdLayout(int N, int L, int C, int K, int pad) {
        Lout = L + 2 * pad - K + 1;
        ctiles = (C + QD_C - 1) / QD_C;
        tiles_t = (Lout + QD_T - 1) / QD_T;
        units = (long)N * tiles_t;
        long b = QD_WORKGROUPS / ctiles;
        if (b < 1) b = 1;
        if (b > units) b = units;
        per_block = (units + b - 1) / b;
        blocks = (units + per_block - 1) / per_block;
        part = 0;
        total = align_up256(part + (size_t)blocks * C * K * sizeof(float));
    }
};

struct QdArgs {
    const half_t* x;     // [N][L][C]
    const float* w;      // [C][K]
    const half_t* dy;    // [N][Lout][C]
    half_t* dx;          // [N][L][C]
    float* part;         // [blocks][C][K]
    long units, per_block;
    int L, Lout, C, K, pad, tiles_t;
};

// dx[n][p][c] = sum_k w[c][k] dy[n][p + pad - k][c]; LDS row r holds dy position p0 + pad - (K - 1) + r
__global__ __launch_bounds__(256) void qd_dx_kernel(QdArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int span = QD_T + p.K - 1;
    half_t* ds = (half_t*)smem;                            // [span][QD_C]
    float* ws = (float*)(ds + (size_t)span * QD_C);        // [K][QD_C]
    const long unit = blockIdx.x;
    const int tiles = (p.L + QD_T - 1) / QD_T;
    const long n = unit / tiles;
    const int p0 = (int)(unit - n * tiles) * QD_T, c0 = blockIdx.y * QD_C, tid = threadIdx.x;
    const int q0 = p0 + p.pad - (p.K - 1);
    const half_t* src = p.dy + n * p.Lout * p.C;
    for (int i = tid; i < span * (QD_C / 8); i += 256) {
        const int r = i / (QD_C / 8), cc = (i % (QD_C / 8)) * 8;
        const int q = q0 + r;
        uint4_t v = {0, 0, 0, 0};
        if (q >= 0 && q < p.Lout && c0 + cc < p.C) v = *(const uint4_t*)(src + (long)q * p.C + c0 + cc);
        *(uint4_t*)(ds + r * QD_C + cc) = v;
    }
    for (int i = tid; i < p.K * QD_C; i += 256) {
        const int k = i / QD_C, c = i % QD_C;
        ws[i] = c0 + c < p.C ? p.w[(long)(c0 + c) * p.K + k] : 0.0f;
    }
    __syncthreads();
    const int cc = (tid & 7) * 8;
    if (c0 + cc >= p.C) return;
    for (int tt = tid >> 3; tt < QD_T; tt += 32) {
        const int pos = p0 + tt;
        if (pos >= p.L) break;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const half_t* dr = ds + (tt + p.K - 1) * QD_C + cc;
        for (int k = 0; k < p.K; ++k) {
            const half8_t dv = *(const half8_t*)(dr - k * QD_C);
            const float* wk = ws + k * QD_C + cc;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(wk[e], (float)dv[e], acc[e]);
        }
        half8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)acc[e];
        *(half8_t*)(p.dx + (n * p.L + pos) * p.C + c0 + cc) = o;
    }
}

// part[block][c][k] = sum over the block's units of dy[n][t][c] x[n][t + k - pad][c]; LDS x row r holds position t0 - pad + r, so the row
// of output t0 + tt and tap k is tt + k
template <int KG>
__global__ __launch_bounds__(256) void qd_dw_kernel(QdArgs p) {
    constexpr int XROWS = QD_T + 4 * KG + QD_TB;           // rows a window may touch (zeros behind the halo)
    __shared__ __attribute__((aligned(16))) half_t xs[XROWS * QD_C];
    __shared__ __attribute__((aligned(16))) half_t ds[QD_T * QD_C];
    const int tid = threadIdx.x, c = tid & (QD_C - 1), k0 = (tid >> 6) * KG, c0 = blockIdx.y * QD_C;
    const long u_lo = (long)blockIdx.x * p.per_block, u_hi = u_lo + p.per_block < p.units ? u_lo + p.per_block : p.units;
    float acc[KG];
#pragma unroll
    for (int j = 0; j < KG; ++j) acc[j] = 0.0f;
    for (long u = u_lo; u < u_hi; ++u) {
        const long n = u / p.tiles_t;
        const int t0 = (int)(u - n * p.tiles_t) * QD_T;
        const half_t* xsrc = p.x + n * p.L * p.C;
        const half_t* dsrc = p.dy + n * p.Lout * p.C;
        __syncthreads();                                   // the previous unit has been read
        for (int i = tid; i < XROWS * (QD_C / 8); i += 256) {
            const int r = i / (QD_C / 8), cc = (i % (QD_C / 8)) * 8;
            const int q = t0 - p.pad + r;
            uint4_t v = {0, 0, 0, 0};
            if (r < QD_T + p.K - 1 && q >= 0 && q < p.L && c0 + cc < p.C) v = *(const uint4_t*)(xsrc + (long)q * p.C + c0 + cc);
            *(uint4_t*)(xs + r * QD_C + cc) = v;
        }
        for (int i = tid; i < QD_T * (QD_C / 8); i += 256) {
            const int r = i / (QD_C / 8), cc = (i % (QD_C / 8)) * 8;
            const int t = t0 + r;
            uint4_t v = {0, 0, 0, 0};
            if (t < p.Lout && c0 + cc < p.C) v = *(const uint4_t*)(dsrc + (long)t * p.C + c0 + cc);
            *(uint4_t*)(ds + r * QD_C + cc) = v;
        }
        __syncthreads();
        const int rows = p.Lout - t0 < QD_T ? p.Lout - t0 : QD_T;
        for (int tb = 0; tb < rows; tb += QD_TB) {
            float xw[KG + QD_TB - 1], dv[QD_TB];
#pragma unroll
            for (int j = 0; j < KG + QD_TB - 1; ++j) xw[j] = (float)xs[(tb + k0 + j) * QD_C + c];
#pragma unroll
            for (int i = 0; i < QD_TB; ++i) dv[i] = (float)ds[(tb + i) * QD_C + c];
#pragma unroll
            for (int i = 0; i < QD_TB; ++i)
#pragma unroll
                for (int j = 0; j < KG; ++j) acc[j] = fmaf(dv[i], xw[i + j], acc[j]);
        }
    }
    if (c0 + c < p.C) {
        float* out = p.part + ((long)blockIdx.x * p.C + c0 + c) * p.K;
#pragma unroll
        for (int j = 0; j < KG; ++j)
            if (k0 + j < p.K) out[k0 + j] = acc[j];
    }
}

// out[col] = the blocks' planes [blocks][cols] added in block order
__global__ __launch_bounds__(BS_COLS * BS_RUNS) void q_finish_kernel(const float* __restrict__ part, long blocks, int cols,
                                                                      float* __restrict__ out) {
    __shared__ float run[BS_RUNS][BS_COLS];
    const int col = blockIdx.x * BS_COLS + threadIdx.x % BS_COLS;
    const float s = block_order_sum(part, blocks, cols, col, run);
    if (threadIdx.x < BS_COLS && col < cols) out[col] = s;
}

template <int KG>
void qd_dw_launch(const QdArgs& a, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL(qd_dw_kernel<KG>, grid, dim3(256), 0, stream, a);
}

// ---- residual add + activation + dropout ------------------------------------------------------------------------------------------------------
constexpr unsigned long long Q_GOLDEN = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ unsigned long long q_mix(unsigned long long z) {      // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// key = q_mix(seed + GOLDEN (stream_id + 1)), once per call on the host; an element is kept iff the top 32 bits reach the threshold
__device__ __forceinline__ bool q_keep(unsigned long long key, unsigned long long index, unsigned int threshold) {
    return (unsigned int)(q_mix(key + Q_GOLDEN * (index + 1ull)) >> 32) >= threshold;
}

struct QrArgs {
    const half_t* a;
    const half_t* b;       // or null
    const half_t* dy;      // backward
    half_t* out;           // forward: y;  backward: da
    long vectors;          // M C / 8
    unsigned long long key;
    unsigned int threshold;
    float inv_keep;
    int act;
};

template <bool BACKWARD>
__global__ __launch_bounds__(256) void qr_kernel(QrArgs p) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= p.vectors) return;
    const long e0 = v * 8;
    const half8_t av = *(const half8_t*)(p.a + e0);
    half8_t bv = {0, 0, 0, 0, 0, 0, 0, 0}, dv = {0, 0, 0, 0, 0, 0, 0, 0}, o;
    if (p.b) bv = *(const half8_t*)(p.b + e0);
    if (BACKWARD) dv = *(const half8_t*)(p.dy + e0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float u = p.b ? (float)av[j] + (float)bv[j] : (float)av[j];
        const bool keep = p.threshold == 0u || q_keep(p.key, (unsigned long long)(e0 + j), p.threshold);
        float r;
        if (BACKWARD) r = keep ? (float)dv[j] * p.inv_keep * act_grad(u, p.act) : 0.0f;
        else r = keep ? apply_act_rt(u, p.act) * p.inv_keep : 0.0f;
        o[j] = (half_t)r;
    }
    *(half8_t*)(p.out + e0) = o;
}

// ---- CTC head backward ---------------------------------------------------------------------------------------------------------------------------
constexpr long QH_MIN_ROWS = 64;
constexpr long QH_MAX_BLOCKS = 1024;

inline long qh_block_rows(long M) {
    const long rows = (M + QH_MAX_BLOCKS - 1) / QH_MAX_BLOCKS;
    return rows < QH_MIN_ROWS ? QH_MIN_ROWS : rows;
}

const char* qh_shape_error(long M, int F, int classes) {
    if (M < 1) return "M must be positive";
    if (classes < 1 || classes > 8) return "classes must be in 1..8";
    if (F < 8 || F % 8 != 0) return "F must be a multiple of 8";
    if ((size_t)classes * F * sizeof(float) > 64 * 1024) return "the fp32 weights do not fit 64 KiB of LDS";
    return nullptr;
}

struct QhLayout {
    long rows, blocks;
    int cols;                          // classes (F + 1): dw's columns and, behind each row of them, db
    size_t dlogit, part, sums, total;  // dlogit: fp32 [M][8];  part: fp32 [blocks][cols];  sums: fp32 [cols]
    QhLayout(long M, int F, int classes) {
        rows = qh_block_rows(M);
        blocks = (M + rows - 1) / rows;
        cols = classes * (F + 1);
        dlogit = 0;
        part = align_up256(dlogit + (size_t)M * 8 * sizeof(float));
        sums = align_up256(part + (size_t)blocks * cols * sizeof(float));
        total = align_up256(sums + (size_t)cols * sizeof(float));
    }
};

struct QhArgs {
    const half_t* x;      // [M][F]
    const float* w;       // [classes][F]
    const float* b;       // [classes]
    const half_t* dlp;    // [M][classes]
    half_t* dx;           // [M][F] or null
    float* dlogit;        // [M][8]
    float* part;          // [blocks][classes][F + 1]
    long M, rows;
    int F, classes;
};

// one row per thread: the logits and lse as ctc_head_kernel forms them, dlogit_c = dlp_c - s_c sum dlp, dx = sum_c dlogit_c w[c][.]
__global__ __launch_bounds__(256) void qh_rows_kernel(QhArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ws = (float*)smem;   // [classes][F]
    for (int i = threadIdx.x; i < p.classes * p.F; i += 256) ws[i] = p.w[i];
    __syncthreads();
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= p.M) return;
    float logit[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) logit[c] = (c < p.classes) ? p.b[c] : -INFINITY;
    const half_t* x = p.x + m * p.F;
    for (int f = 0; f < p.F; f += 8) {
        const half8_t xv = *(const half8_t*)(x + f);
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < p.classes) {
                const float* wc = ws + c * p.F + f;
#pragma unroll
                for (int e = 0; e < 8; ++e) logit[c] = fmaf(wc[e], (float)xv[e], logit[c]);
            }
    }
    float mx = logit[0];
#pragma unroll
    for (int c = 1; c < 8; ++c) mx = fmaxf(mx, logit[c]);
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) sum += (c < p.classes) ? __expf(logit[c] - mx) : 0.0f;
    const float lse = mx + __logf(sum);
    float d[8], g = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        d[c] = c < p.classes ? (float)p.dlp[m * p.classes + c] : 0.0f;
        g += d[c];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        d[c] = c < p.classes ? d[c] - __expf(logit[c] - lse) * g : 0.0f;
        p.dlogit[m * 8 + c] = d[c];
    }
    if (!p.dx) return;
    half_t* dx = p.dx + m * p.F;
    for (int f = 0; f < p.F; f += 8) {
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < p.classes) {
                const float* wc = ws + c * p.F + f;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(d[c], wc[e], acc[e]);
            }
        half8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)acc[e];
        *(half8_t*)(dx + f) = o;
    }
}

// part[block][c][f] = sum over the block's rows of dlogit[m][c] x[m][f], f < F; column F: x = 1 (db)
__global__ __launch_bounds__(256) void qh_dw_kernel(QhArgs p) {
    const long r_lo = (long)blockIdx.x * p.rows, r_hi = r_lo + p.rows < p.M ? r_lo + p.rows : p.M;
    float* out = p.part + (long)blockIdx.x * p.classes * (p.F + 1);
    for (int f = threadIdx.x; f <= p.F; f += 256) {
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (long m = r_lo; m < r_hi; ++m) {
            const float xv = f < p.F ? (float)p.x[m * p.F + f] : 1.0f;
            const float4_t d0 = *(const float4_t*)(p.dlogit + m * 8), d1 = *(const float4_t*)(p.dlogit + m * 8 + 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[c] = fmaf(d0[c], xv, acc[c]);
                acc[4 + c] = fmaf(d1[c], xv, acc[4 + c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < p.classes) out[c * (p.F + 1) + f] = acc[c];
    }
}

// sums [classes][F + 1] -> dw [classes][F] and db [classes], each where asked for
__global__ __launch_bounds__(256) void qh_scatter_kernel(const float* __restrict__ sums, int F, int classes, float* __restrict__ dw,
                                                         float* __restrict__ db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= classes * (F + 1)) return;
    const int c = i / (F + 1), f = i - c * (F + 1);
    if (f < F) {
        if (dw) dw[c * F + f] = sums[i];
    } else if (db) db[c] = sums[i];
}

}  // namespace
}  // namespace bh

size_t bh_k_dwconv_train_workspace(int N, int L, int C, int K, int pad) {
    return bh::qd_shape_error(N, L, C, K, pad) ? 0 : bh::QdLayout(N, L, C, K, pad).total;
}

int bh_k_dwconv_train_backward(const void* x, const float* w, const void* dy, int N, int L, int C, int K, int pad, void* dx, float* dw,
                               void* workspace, size_t workspace_bytes, hipStream_t stream) {
    using namespace bh;
    const char* shape_err = qd_shape_error(N, L, C, K, pad);
    BH_REQUIRE(!shape_err, "dwconv1d_train_backward: %s (N=%d L=%d C=%d K=%d pad=%d)", shape_err, N, L, C, K, pad);
    const QdLayout lay(N, L, C, K, pad);
    BH_REQUIRE(workspace_bytes >= lay.total, "dwconv1d_train_backward: workspace of %zu bytes, bh_dwconv1d_train_workspace = %zu",
               workspace_bytes, lay.total);
    BH_REQUIRE(x && w && dy && workspace, "dwconv1d_train_backward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(workspace),
               "dwconv1d_train_backward: x, dy, dx and workspace must be 16-byte aligned");
    const long dx_units = (long)N * ((L + QD_T - 1) / QD_T);
    BH_REQUIRE(dx_units < (1l << 24) && lay.units < (1l << 24), "dwconv1d_train_backward: N L must stay below 2^30 rows");
    float* part = (float*)((char*)workspace + lay.part);
    const QdArgs a{(const half_t*)x, w, (const half_t*)dy, (half_t*)dx, part, lay.units, lay.per_block, L, lay.Lout, C, K, pad, lay.tiles_t};
    if (dx) {
        const size_t lds = (size_t)(QD_T + K - 1) * QD_C * sizeof(half_t) + (size_t)K * QD_C * sizeof(float);     // <= 56.3 KiB at K = 127
        hipLaunchKernelGGL(qd_dx_kernel, dim3((unsigned)dx_units, lay.ctiles), dim3(256), lds, stream, a);
    }
    if (dw) {
        const dim3 grid((unsigned)lay.blocks, lay.ctiles);
        switch (qd_tap_group(K)) {
            case 1: qd_dw_launch<1>(a, grid, stream); break;
            case 2: qd_dw_launch<2>(a, grid, stream); break;
            case 4: qd_dw_launch<4>(a, grid, stream); break;
            case 8: qd_dw_launch<8>(a, grid, stream); break;
            case 16: qd_dw_launch<16>(a, grid, stream); break;
            default: qd_dw_launch<32>(a, grid, stream); break;
        }
        const int cols = C * K;
        hipLaunchKernelGGL(q_finish_kernel, dim3((cols + BS_COLS - 1) / BS_COLS), dim3(BS_COLS * BS_RUNS), 0, stream, (const float*)part,
                           lay.blocks, cols, dw);
    }
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

static int residual_act_launch(bool backward, const void* a, const void* b, const void* dy, long M, int C, int act, unsigned int p_threshold,
                               float inv_keep, unsigned long long seed, unsigned long long stream_id, void* out, hipStream_t stream) {
    using namespace bh;
    const char* what = backward ? "residual_act_train_backward" : "residual_act_train_forward";
    BH_REQUIRE(M >= 1 && C >= 8 && C % 8 == 0, "%s: M must be positive and C a multiple of 8 (M=%ld C=%d)", what, M, C);
    BH_REQUIRE(act_ok(act), "%s: unknown activation %d", what, act);
    BH_REQUIRE(std::isfinite(inv_keep) && inv_keep >= 1.0f, "%s: inv_keep = 1 / (1 - p) must be finite and >= 1 (got %g)", what,
               (double)inv_keep);
    BH_REQUIRE(a && out && (!backward || dy), "%s: null pointer", what);
    BH_REQUIRE(aligned16(a) && aligned16(b) && aligned16(dy) && aligned16(out), "%s: every pointer must be 16-byte aligned", what);
    const long vectors = M * (C / 8), grid = (vectors + 255) / 256;
    BH_REQUIRE(grid < (1l << 24), "%s: M C must stay below 2^35 elements", what);
    const QrArgs q{(const half_t*)a, (const half_t*)b, (const half_t*)dy, (half_t*)out, vectors, q_mix(seed + Q_GOLDEN * (stream_id + 1ull)),
                   p_threshold, inv_keep, act};
    if (backward) hipLaunchKernelGGL(qr_kernel<true>, dim3((unsigned)grid), dim3(256), 0, stream, q);
    else hipLaunchKernelGGL(qr_kernel<false>, dim3((unsigned)grid), dim3(256), 0, stream, q);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

int bh_k_residual_act_train_forward(const void* a, const void* b, long M, int C, int act, unsigned int p_threshold, float inv_keep,
                                    unsigned long long seed, unsigned long long stream_id, void* y, hipStream_t stream) {
    return residual_act_launch(false, a, b, nullptr, M, C, act, p_threshold, inv_keep, seed, stream_id, y, stream);
}

int bh_k_residual_act_train_backward(const void* a, const void* b, const void* dy, long M, int C, int act, unsigned int p_threshold,
                                     float inv_keep, unsigned long long seed, unsigned long long stream_id, void* da, hipStream_t stream) {
    return residual_act_launch(true, a, b, dy, M, C, act, p_threshold, inv_keep, seed, stream_id, da, stream);
}

size_t bh_k_ctc_head_train_workspace(long M, int F, int classes) {
    return bh::qh_shape_error(M, F, classes) ? 0 : bh::QhLayout(M, F, classes).total;
}

int bh_k_ctc_head_train_backward(const void* x, const float* w, const float* bias, const void* dlp, long M, int F, int classes, void* dx,
                                 float* dw, float* db, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    using namespace bh;
    const char* shape_err = qh_shape_error(M, F, classes);
    BH_REQUIRE(!shape_err, "ctc_head_train_backward: %s (M=%ld F=%d classes=%d)", shape_err, M, F, classes);
    const QhLayout lay(M, F, classes);
    BH_REQUIRE(workspace_bytes >= lay.total, "ctc_head_train_backward: workspace of %zu bytes, bh_ctc_head_train_workspace = %zu",
               workspace_bytes, lay.total);
    BH_REQUIRE(x && w && bias && dlp && workspace, "ctc_head_train_backward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(dx) && aligned16(workspace), "ctc_head_train_backward: x, dx and workspace must be 16-byte aligned");
    const long row_grid = (M + 255) / 256;
    BH_REQUIRE(row_grid < (1l << 24), "ctc_head_train_backward: M must stay below 2^32 rows");
    float* dlogit = (float*)((char*)workspace + lay.dlogit);
    float* part = (float*)((char*)workspace + lay.part);
    float* sums = (float*)((char*)workspace + lay.sums);
    const QhArgs a{(const half_t*)x, w, bias, (const half_t*)dlp, (half_t*)dx, dlogit, part, M, lay.rows, F, classes};
    hipLaunchKernelGGL(qh_rows_kernel, dim3((unsigned)row_grid), dim3(256), (size_t)classes * F * sizeof(float), stream, a);
    if (dw || db) {
        hipLaunchKernelGGL(qh_dw_kernel, dim3((unsigned)lay.blocks), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(q_finish_kernel, dim3((lay.cols + BS_COLS - 1) / BS_COLS), dim3(BS_COLS * BS_RUNS), 0, stream, (const float*)part,
                           lay.blocks, lay.cols, sums);
        hipLaunchKernelGGL(qh_scatter_kernel, dim3((lay.cols + 255) / 256), dim3(256), 0, stream, (const float*)sums, F, classes, dw, db);
    }
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
