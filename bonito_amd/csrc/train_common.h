// What the training units share (lstm_train.hip, train_layers.hip, transformer_train.hip): the small host helpers, the split of a
// reduction over rows, and the three entries of train_common.hip - reduce_rows (the weight and bias gradients of every layer),
// round_weights (a linear layer's fp32 master weights as the fp16 operand of a launch) and linear_rows (a GEMM over all T N rows
// through bh_k_linear). Each exists once; the kernels are compiled in train_common.hip only.
#pragma once
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace bh {

// LDS and workspace bytes written as halves and read back as vectors (or the reverse) go through may_alias types
typedef half8_t __attribute__((may_alias)) half8_alias_t;
typedef half_t __attribute__((may_alias)) half_alias_t;

inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }
// grid of a grid-stride conversion kernel of 256 threads over n elements
inline int cvt_grid(long n) { return (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024); }

// ---- activation, its derivative and the clamp's mask ------------------------------------------------------------------------------------
inline bool act_ok(int act) { return act == ACT_NONE || act == ACT_SWISH || act == ACT_TANH || act == ACT_RELU; }
inline bool is_clamped(float lo, float hi) { return !(lo == -INFINITY && hi == INFINITY); }
__device__ __forceinline__ float act_grad(float z, int act) {
    switch (act) {
        case ACT_SWISH: { const float s = sigmoidf_(z); return s * (1.0f + z * (1.0f - s)); }
        case ACT_TANH: { const float t = tanhf_(z); return 1.0f - t * t; }
        case ACT_RELU: return z > 0.0f ? 1.0f : 0.0f;
        default: return 1.0f;
    }
}

// One column of partial sums [blocks][C], added in block order by a workgroup of BS_COLS x BS_RUNS threads (thread = column
// threadIdx.x % BS_COLS, run threadIdx.x / BS_COLS): the blocks are cut into BS_RUNS runs of consecutive blocks (a function of their
// number alone), a thread adds one run of its column in block order - eight loads in flight, the additions in order - and the runs are
// added in run order. -> the sum, in the threads of run 0 (the others get their run's sum). run: LDS, free again after the call.
constexpr int BS_COLS = 32, BS_RUNS = 8;
__device__ __forceinline__ float block_order_sum(const float* __restrict__ part, long blocks, int C, int c, float (*run)[BS_COLS]) {
    const int col = threadIdx.x % BS_COLS, g = threadIdx.x / BS_COLS;
    const long per = (blocks + BS_RUNS - 1) / BS_RUNS;
    const long b_lo = g * per, b_hi = b_lo + per < blocks ? b_lo + per : blocks;
    float s = 0.0f;
    if (c < C) {
        long b = b_lo;
        for (; b + 8 <= b_hi; b += 8) {
            float t[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) t[i] = part[(b + i) * C + c];
#pragma unroll
            for (int i = 0; i < 8; ++i) s += t[i];
        }
        for (; b < b_hi; ++b) s += part[b * C + c];
    }
    __syncthreads();
    run[g][col] = s;
    __syncthreads();
    if (g == 0) {
        s = run[0][col];
#pragma unroll
        for (int q = 1; q < BS_RUNS; ++q) s += run[q][col];
    }
    return s;
}

// ---- the reduction over rows: dw = A^T B, db = column sums of A ------------------------------------------------------------------------
constexpr int RT_TILE = 64;            // atb kernel: 64 x 64 outputs per workgroup
constexpr int RT_KSTEP = 32;           // rows of M per MFMA

// how the M rows are split: a function of the shape alone (the order of the sums never varies)
struct Split {
    int dw_splits, db_splits;
    long dw_rows, db_rows;       // rows per block (dw_rows a multiple of RT_KSTEP)
    Split(long M, int R, int Cc) {
        const long tiles = (long)((R + RT_TILE - 1) / RT_TILE) * ((Cc + RT_TILE - 1) / RT_TILE);
        long s = (M + 511) / 512;
        const long cap = tiles >= 1024 ? 1 : 1024 / tiles;
        if (s > cap) s = cap;
        if (s < 1) s = 1;
        long rows = ((M + s - 1) / s + RT_KSTEP - 1) / RT_KSTEP * RT_KSTEP;
        dw_splits = (int)((M + rows - 1) / rows);
        dw_rows = rows;
        long b = (M + 255) / 256;
        if (b > 1024) b = 1024;
        rows = (M + b - 1) / b;
        db_splits = (int)((M + rows - 1) / rows);
        db_rows = rows;
    }
};

// where row m of B lies, and with it where the reduced sums go
enum RowKind : int {
    ROWS_PLAIN = 0,     // b + m * ld (ld % 8 == 0);  dw [R][Cc]
    ROWS_CONV = 1,      // the window of position t = m % Lout of chunk n = m / Lout, zero over an edge;  dw [R][Cin][K]
    ROWS_LSTM = 2       // [x[m] | h[tp(m)]], m = t N + n, tp = t + 1 (reverse) or t - 1, zeros where tp leaves 0..T-1;
                        // columns below H to dw [R][H], the rest to dw_hi [R][H]
};
struct RowRule {
    const half_t* b;
    int kind;
    long ld;                           // plain: the row pitch.  LSTM: H (b = x [T][N][H], Cc = 2 H, H % 8 == 0)
    int Lout, Lin, Cin, stride, pad;   // conv: x [N][Lin][Cin], Cin == 1 or Cin % 8 == 0; column c = k * Cin + ci
    const half_t* h;                   // LSTM: h [T][N][H]
    int T, N, reverse;
};

// dw (and dw_hi) = a^T B and, where db is not null, db = column sums of a [M][R] (R % 4 == 0); the partial sums of the blocks go to
// dw_part [Split::dw_splits][R][Cc] / db_part [Split::db_splits][R] and are added in block order
int reduce_rows(const half_t* a, const RowRule& b, long M, int R, int Cc, float* dw_part, float* db_part, float* dw, float* dw_hi, float* db,
                hipStream_t stream);

// ---- the master weights of a linear layer, rounded ------------------------------------------------------------------------------------------
enum WeightForm : int {
    WEIGHTS_ROWS = 0,         // fp16 [C][K], the rows as they are
    WEIGHTS_TRANSPOSED = 1,   // fp16 [K][C]
    WEIGHTS_GATED_PAIRS = 2   // fp16 [C][K] with row j of the first half at 2 j and row j of the second half at 2 j + 1: (y_j, gate_j), what
                        // bh_k_linear's SwiGLU epilogue reads (C even)
};
// fp32 w [C][K] (a device tensor, torch's layout) -> its round-to-nearest fp16 values in `form`; one launch
int round_weights(const float* w, half_t* out, int C, int K, int form, hipStream_t stream);

// ---- a GEMM over all rows ----------------------------------------------------------------------------------------------------------------
// rows of one bh_k_linear call: its kernels may index an operand with 32-bit offsets, so both stay below 2^30 halves; the rows of a GEMM
// are independent, the blocks change no byte. With the batch-major row map a block is whole time steps (a multiple of N rows).
inline long gemm_rows(int K, int C, int N, bool whole_steps) {
    long rows = (1l << 30) / (K > C ? K : C);
    if (whole_steps) rows = rows / N >= 1 ? rows / N * N : N;
    else rows = rows / 256 >= 1 ? rows / 256 * 256 : rows;
    return rows;
}
// Y = clamp(act(X W^T + b) scale, lo, hi) over the T N rows m = t N + n of x [T][N][K], block by block; y [T][N][C], or batch-major
// [N][T][C]. gated: w's C rows are pairs (y_j, gate_j) and y has C / 2 columns y_j gate_j sigmoid(gate_j), bh_k_linear's SwiGLU epilogue
// (act none, no bias). The first non-zero return code of bh_k_linear is passed up.
int linear_rows(const half_t* x, const half_t* w, const float* bias, half_t* y, int T, int N, int K, int C, int act, float scale, float lo,
                float hi, bool batch_major, bool gated, hipStream_t stream);

}  // namespace bh
