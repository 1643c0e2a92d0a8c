// The pieces the training layers share (train_common.h), on gfx950: the reduction over rows that gives the weight and bias
// gradients, the rounding of a linear layer's master weights, and the loop that walks bh_k_linear over blocks of rows.
//     dW = dz^T B over the M rows and db = sum of dz are ONE kernel family for every layer (atb_kernel + colsum_kernel + reduce_kernel).
//     B's row m (RowRule) is X[m] for the linear layer; for the convolution the window of K Cin contiguous halves at x[n][t s - p], zero
//     where it hangs over an edge; for the LSTM layer [x[m] | h of the step processed before m's], zero at the first processed step.
//     Both operands are transposed through LDS into v_mfma_f32_16x16x32_f16 with 32 rows as k. The rows are split into blocks (Split)
//     whose partial sums a second kernel adds IN BLOCK ORDER: no floating-point atomics, equal bytes from call to call. The rule kind
//     is a template parameter: an instance pays for its own rule only.
// Every kernel of this file indexes with 64 bits.
#include "train_common.h"

namespace bh {
namespace {

constexpr int RT_LD = RT_KSTEP + 8;    // LDS row pitch in halves (80 bytes: 16-byte aligned, off the power of two)
constexpr int DB_THREADS = 128;

template <int KIND>
__device__ __forceinline__ half8_t load_b8(const RowRule& r, long m, int c8, int Cc) {
    half8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c8 >= Cc) return v;
    if constexpr (KIND == ROWS_PLAIN) return *(const half8_t*)(r.b + m * r.ld + c8);
    if constexpr (KIND == ROWS_LSTM) {      // H % 8 == 0: a vector lies in x or in h, never across
        if (c8 < r.ld) return *(const half8_t*)(r.b + m * r.ld + c8);
        const long t = m / r.N, tp = r.reverse ? t + 1 : t - 1;
        if (tp < 0 || tp >= r.T) return v;
        return *(const half8_t*)(r.h + (m + (tp - t) * r.N) * r.ld + (c8 - r.ld));
    }
    const long n = m / r.Lout;
    const int t = (int)(m - n * r.Lout);
    if (r.Cin == 1) {
        const half_t* x = r.b + n * r.Lin;
        const int l0 = t * r.stride - r.pad + c8;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c8 + j < Cc && l0 + j >= 0 && l0 + j < r.Lin) v[j] = x[l0 + j];
        return v;
    }
    const int k = c8 / r.Cin, ci = c8 - k * r.Cin;      // Cin % 8 == 0: the vector lies in one input position
    const int l = t * r.stride - r.pad + k;
    if (l < 0 || l >= r.Lin) return v;
    return *(const half8_t*)(r.b + (n * r.Lin + l) * r.Cin + ci);
}

struct AtbArgs {
    const half_t* a;        // [M][R], R % 4 == 0
    RowRule b;
    float* part;            // [splits][R][Cc]
    long M, rows;
    int R, Cc;
};

// part[z][r][c] = sum over the rows m of block z of a[m][r] * B[m][c]   (both operands transposed through LDS)
template <int KIND>
__global__ __launch_bounds__(256) void atb_kernel(AtbArgs p) {
    __shared__ __attribute__((aligned(16))) half_t At[RT_TILE * RT_LD];
    __shared__ __attribute__((aligned(16))) half_t Bt[RT_TILE * RT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = p.R, Cc = p.Cc;
    const int r0 = blockIdx.x * RT_TILE, c0 = blockIdx.y * RT_TILE;
    const long m_lo = (long)blockIdx.z * p.rows, m_hi = m_lo + p.rows < p.M ? m_lo + p.rows : p.M;
    const int mm = tid >> 3, v = tid & 7;
    const int r8 = r0 + v * 8, c8 = c0 + v * 8;
    float4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
    for (long m0 = m_lo; m0 < m_hi; m0 += RT_KSTEP) {
        const long m = m0 + mm;
        half8_t a8 = {0, 0, 0, 0, 0, 0, 0, 0}, b8 = {0, 0, 0, 0, 0, 0, 0, 0};
        if (m < m_hi) {
            const half_t* ar = p.a + m * R + r8;
            if ((R & 7) == 0) {
                if (r8 < R) a8 = *(const half8_t*)ar;
            } else {
                if (r8 < R) { const half4_t lo = *(const half4_t*)ar; a8[0] = lo[0]; a8[1] = lo[1]; a8[2] = lo[2]; a8[3] = lo[3]; }
                if (r8 + 4 < R) { const half4_t hi = *(const half4_t*)(ar + 4); a8[4] = hi[0]; a8[5] = hi[1]; a8[6] = hi[2]; a8[7] = hi[3]; }
            }
            b8 = load_b8<KIND>(p.b, m, c8, Cc);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ((half_alias_t*)At)[(v * 8 + j) * RT_LD + mm] = a8[j];
            ((half_alias_t*)Bt)[(v * 8 + j) * RT_LD + mm] = b8[j];
        }
        __syncthreads();
        const half8_t a = *(const half8_alias_t*)(At + (wave * 16 + (lane & 15)) * RT_LD + (lane >> 4) * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[j] = mfma16(a, *(const half8_alias_t*)(Bt + (j * 16 + (lane & 15)) * RT_LD + (lane >> 4) * 8), acc[j]);
        __syncthreads();
    }
    float* out = p.part + (long)blockIdx.z * R * Cc;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + wave * 16 + (lane >> 4) * 4 + i, c = c0 + j * 16 + (lane & 15);
            if (r < R && c < Cc) out[(long)r * Cc + c] = acc[j][i];
        }
}

// part[z][r] = sum over the rows of block z of a[m][r]
__global__ __launch_bounds__(DB_THREADS) void colsum_kernel(const half_t* __restrict__ a, float* __restrict__ part, long M, int R, long rows) {
    const int r = blockIdx.x * DB_THREADS + threadIdx.x;
    if (r >= R) return;
    const long m_lo = (long)blockIdx.y * rows, m_hi = m_lo + rows < M ? m_lo + rows : M;
    float s = 0.0f;
    for (long m = m_lo; m < m_hi; ++m) s += (float)a[m * R + r];
    part[(long)blockIdx.y * R + r] = s;
}

// the partial sums in the order of the blocks, stored as the rule kind says (convolution: column c = k Cin + ci)
template <int KIND>
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ part, int splits, const float* __restrict__ dbp, int db_splits,
                                                     int R, int Cc, int Cin, int K, float* __restrict__ dw, float* __restrict__ dw_hi,
                                                     float* __restrict__ db) {
    const long nw = (long)R * Cc;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nw) {
        float s = part[e];
        for (int z = 1; z < splits; ++z) s += part[z * nw + e];
        if constexpr (KIND == ROWS_PLAIN) {
            dw[e] = s;
        } else {
            const long r = e / Cc;
            const int c = (int)(e - r * Cc);
            if constexpr (KIND == ROWS_CONV) {
                const int k = c / Cin, ci = c - k * Cin;
                dw[(r * Cin + ci) * K + k] = s;
            } else {
                const int H = Cc / 2;
                if (c < H) dw[r * H + c] = s;
                else dw_hi[r * H + c - H] = s;
            }
        }
    } else if (db && e < nw + R) {
        const long r = e - nw;
        float s = dbp[r];
        for (int z = 1; z < db_splits; ++z) s += dbp[(long)z * R + r];
        db[r] = s;
    }
}

template <int KIND>
int reduce_rows_of(const half_t* a, const RowRule& b, long M, int R, int Cc, float* dw_part, float* db_part, float* dw, float* dw_hi, float* db,
                   hipStream_t stream) {
    const Split g(M, R, Cc);
    AtbArgs d{a, b, dw_part, M, g.dw_rows, R, Cc};
    hipLaunchKernelGGL(atb_kernel<KIND>, dim3((R + RT_TILE - 1) / RT_TILE, (Cc + RT_TILE - 1) / RT_TILE, g.dw_splits), dim3(256), 0, stream, d);
    if (db)
        hipLaunchKernelGGL(colsum_kernel, dim3((R + DB_THREADS - 1) / DB_THREADS, g.db_splits), dim3(DB_THREADS), 0, stream, a, db_part, M, R,
                           g.db_rows);
    const long outputs = (long)R * Cc + R;
    hipLaunchKernelGGL(reduce_kernel<KIND>, dim3((unsigned)((outputs + 255) / 256)), dim3(256), 0, stream, dw_part, g.dw_splits, db_part,
                       g.db_splits, R, Cc, b.Cin, b.Cin ? Cc / b.Cin : 0, dw, dw_hi, db);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void round_weights_kernel(const float* __restrict__ w, half_t* __restrict__ out, int C, int K, int form) {
    const long total = (long)C * K;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long c = e / K, k = e - c * K;
        long to = e;
        if (form == WEIGHTS_TRANSPOSED) to = k * C + c;
        else if (form == WEIGHTS_GATED_PAIRS) to = (c < C / 2 ? 2 * c : 2 * (c - C / 2) + 1) * K + k;
        out[to] = (half_t)w[e];
    }
}

}  // namespace

int round_weights(const float* w, half_t* out, int C, int K, int form, hipStream_t stream) {
    hipLaunchKernelGGL(round_weights_kernel, dim3(cvt_grid((long)C * K)), dim3(256), 0, stream, w, out, C, K, form);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

int reduce_rows(const half_t* a, const RowRule& b, long M, int R, int Cc, float* dw_part, float* db_part, float* dw, float* dw_hi, float* db,
                hipStream_t stream) {
    switch (b.kind) {
        case ROWS_PLAIN: return reduce_rows_of<ROWS_PLAIN>(a, b, M, R, Cc, dw_part, db_part, dw, dw_hi, db, stream);
        case ROWS_CONV: return reduce_rows_of<ROWS_CONV>(a, b, M, R, Cc, dw_part, db_part, dw, dw_hi, db, stream);
        case ROWS_LSTM: return reduce_rows_of<ROWS_LSTM>(a, b, M, R, Cc, dw_part, db_part, dw, dw_hi, db, stream);
    }
    bh_set_error("reduce_rows: unknown row rule %d", b.kind);
    return -2;
}

int linear_rows(const half_t* x, const half_t* w, const float* bias, half_t* y, int T, int N, int K, int C, int act, float scale, float lo,
                float hi, bool batch_major, bool gated, hipStream_t stream) {
    const long rows = (long)T * N, step = gemm_rows(K, C, N, batch_major);
    const int ldo = gated ? C / 2 : C;      // the SwiGLU epilogue stores one column per (y_j, gate_j) pair of W's rows
    for (long m0 = 0; m0 < rows; m0 += step) {
        const int m = (int)(rows - m0 < step ? rows - m0 : step);
        int rc;
        if (batch_major)      // rows are (t, n): the engine's remap to [N][T][C]; the block starts at time step m0 / N
            rc = bh_k_linear(x + m0 * K, w, bias, y + m0 / N * ldo, m, C, K, K, K, ldo, act, scale, lo, hi, gated, N, 1, T, N, stream);
        else
            rc = bh_k_linear(x + m0 * K, w, bias, y + m0 * ldo, m, C, K, K, K, ldo, act, scale, lo, hi, gated, 0, 0, 0, 0, stream);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace bh
