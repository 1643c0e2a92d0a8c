// Batch-statistics BatchNorm for TRAINING on gfx950: what follows z = conv(x) in a normalised convolution (the reference's
// Convolution.forward is activation(norm(conv(x))); torch.nn.BatchNorm1d in training mode).
//     y = clamp(act(u), lo, hi)     u = gamma xh + beta     xh = (z - mean_c) rstd_c     rstd = 1 / sqrt(var + eps)
// mean_c and the biased var_c over the M = N L rows of channel c. The layouts are those of train_layers.hip: z fp16 [N][L][C]
// channel-minor (C % 8 == 0), y at n os_n + t os_t + c (the permute in front of an LSTM folds into the store), dy in y's layout, dz in
// z's row order. gamma and beta are fp32 and used unrounded (autocast leaves batch-norm parameters in fp32). Channels c >= C_param are
// the zero padding forward_train adds: y = 0 and dz = 0 exactly there, and no statistic or parameter is read or written for them.
//
// Every pass has one shape. A workgroup owns a block of consecutive rows (bn_block_rows, a function of M alone). A thread owns one
// 16-byte vector of 8 channels and every rpi-th row of the block (rpi = 256 / (C / 8) rows are in flight per workgroup), so a wave
// reads consecutive bytes. Sums: a thread adds its rows in row order in fp32, the rpi row slots are added in slot order through LDS
// (fold_slots), the blocks in block order by block_order_sum (train_common.h): no floating-point atomics, equal bytes from call to call.
//
// Forward, three reads of z and one write: the sums of z give the mean; a second, CENTRED pass gives var = sum (z - mean)^2 / M
// (E[z^2] - E[z]^2 on raw fp32 values loses every digit of a channel with mean 8 and deviation 0.05); the finishing kernel writes rstd
// and the running statistics (rm <- (1 - mom) rm + mom mean, rv <- (1 - mom) rv + mom var M / (M - 1)) with no host synchronisation;
// the third pass normalises and stores. mean and rstd are kept for the backward.
// Backward, five reads and one write: du = dy [lo < y < hi] act'(u), u recomputed in fp32 from z, mean, rstd; the mask is read from the
// STORED fp16 y (the rule of train_layers.hip). Pass A: dbeta = sum du, dgamma = sum du xh. Pass B:
//     dz = gamma rstd (du - dbeta / M - xh dgamma / M).
// Every kernel of this file indexes with 64 bits.
#include <cmath>

#include "train_common.h"

namespace bh {
namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_C = 2048;           // C / 8 vectors of one row fit one workgroup
constexpr long BN_MIN_ROWS = 64;         // rows of a block, at least
constexpr long BN_MAX_BLOCKS = 2048;

inline long bn_block_rows(long M) {
    const long rows = (M + BN_MAX_BLOCKS - 1) / BN_MAX_BLOCKS;
    return rows < BN_MIN_ROWS ? BN_MIN_ROWS : rows;
}
inline long bn_blocks(long M) { const long rows = bn_block_rows(M); return (M + rows - 1) / rows; }

const char* bn_shape_error(int N, int L, int C, int C_param) {
    if (N < 1 || L < 1) return "N and L must be positive";
    if ((long)N * L < 2) return "more than one value per channel is needed (N L >= 2)";
    if (C < 8 || C % 8 != 0 || C > BN_MAX_C) return "C must be a multiple of 8 up to 2048";
    if (C_param < 1 || C_param > C) return "C_param must be in 1..C";
    return nullptr;
}

struct BnLayout {
    long blocks;
    size_t part, sums, total;      // part: fp32 [2][blocks][C];  sums: fp32 [2][C] (dbeta, dgamma)
    BnLayout(long M, int C) {
        blocks = bn_blocks(M);
        part = 0;
        sums = align_up256(part + (size_t)2 * blocks * C * sizeof(float));
        total = align_up256(sums + (size_t)2 * C * sizeof(float));
    }
};

struct BnArgs {
    const half_t* z;        // [M][C]
    const half_t* y;        // at n os_n + t os_t + c (backward)
    const half_t* dy;       // in y's layout (backward)
    half_t* out;            // forward: y;  backward: dz [M][C]
    const float* gamma;     // [C_param] or null
    const float* beta;
    const float* mean;      // [C_param]
    const float* rstd;
    const float* sums;      // [2][C]: dbeta, dgamma (backward pass B)
    float* part;            // [2][blocks][C]
    long M, rows, blocks, os_n, os_t;
    int L, C, Cp, act, clamped;
    float lo, hi;
};

// the rows of a thread: row = first, first + rpi, ... below r_hi; c0 its first channel. A thread beyond the last whole row slot has none.
struct BnThread {
    int c0, rpi;
    long first, r_hi;
    __device__ __forceinline__ BnThread(long M, long rows, int C) {
        const int cv = C >> 3;
        rpi = BN_THREADS / cv;
        const int slot = threadIdx.x / cv;
        c0 = (threadIdx.x - slot * cv) * 8;
        const long r_lo = (long)blockIdx.x * rows;
        r_hi = r_lo + rows < M ? r_lo + rows : M;
        first = slot < rpi ? r_lo + slot : r_hi;
    }
};

// out[c] = the sum over the workgroup's row slots of acc, in slot order. Below 256 channels the slots are first added in g = 256 / C
// interleaved groups (slot s into group s % g, ascending), then the groups in order.
__device__ __forceinline__ void fold_slots(float* red, const float (&acc)[8], const BnThread& t, int C, float* __restrict__ out) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < t.rpi * (C >> 3)) {
        float* r = red + (tid / (C >> 3)) * C + t.c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = acc[j];
    }
    __syncthreads();
    const int g = C < BN_THREADS ? BN_THREADS / C : 1;
    int left = t.rpi;
    if (g > 1) {
        if (tid < g * C) {
            const int gi = tid / C, c = tid - gi * C;
            float s = red[gi * C + c];
            for (int sl = gi + g; sl < t.rpi; sl += g) s += red[sl * C + c];
            red[gi * C + c] = s;
        }
        __syncthreads();
        left = g < t.rpi ? g : t.rpi;
    }
    for (int c = tid; c < C; c += BN_THREADS) {
        float s = red[c];
        for (int q = 1; q < left; ++q) s += red[q * C + c];
        out[c] = s;
    }
}

// the per-channel values of a thread's 8 channels; a padded channel gets `pad`
__device__ __forceinline__ void load8(float (&v)[8], const float* __restrict__ src, int c0, int Cp, float absent, float pad) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = c0 + j >= Cp ? pad : src ? src[c0 + j] : absent;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// part[block][c] = sum of z over the block's rows
__global__ __launch_bounds__(BN_THREADS) void bn_sum_kernel(BnArgs p) {
    __shared__ float red[BN_THREADS * 8];
    const BnThread t(p.M, p.rows, p.C);
    const half_t* __restrict__ z = p.z;
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (long r = t.first; r < t.r_hi; r += t.rpi) {
        const half8_t v = *(const half8_t*)(z + r * p.C + t.c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
    }
    fold_slots(red, acc, t, p.C, p.part + (long)blockIdx.x * p.C);
}

// part[block][c] = sum of (z - mean_c)^2 over the block's rows
__global__ __launch_bounds__(BN_THREADS) void bn_centred_kernel(BnArgs p) {
    __shared__ float red[BN_THREADS * 8];
    const BnThread t(p.M, p.rows, p.C);
    const half_t* __restrict__ z = p.z;
    float mean[8], acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    load8(mean, p.mean, t.c0, p.Cp, 0.0f, 0.0f);
#pragma unroll 4
    for (long r = t.first; r < t.r_hi; r += t.rpi) {
        const half8_t v = *(const half8_t*)(z + r * p.C + t.c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = (float)v[j] - mean[j];
            acc[j] = fmaf(d, d, acc[j]);
        }
    }
    fold_slots(red, acc, t, p.C, p.part + (long)blockIdx.x * p.C);
}

// mean[c] = the blocks' sums in block order / M
__global__ __launch_bounds__(BS_COLS * BS_RUNS) void bn_mean_kernel(const float* __restrict__ part, long blocks, int C, int Cp, long M,
                                                                     float* __restrict__ mean) {
    __shared__ float run[BS_RUNS][BS_COLS];
    const int c = blockIdx.x * BS_COLS + threadIdx.x % BS_COLS;
    const float s = block_order_sum(part, blocks, C, c, run);
    if (threadIdx.x < BS_COLS && c < Cp) mean[c] = s / (float)M;
}

// var = the blocks' centred sums in block order / M;  rstd[c];  the running statistics where they are tracked
__global__ __launch_bounds__(BS_COLS * BS_RUNS) void bn_rstd_kernel(const float* __restrict__ part, long blocks, int C, int Cp, long M, float eps,
                                                                     float momentum, const float* __restrict__ mean, float* __restrict__ rstd,
                                                                     float* __restrict__ running_mean, float* __restrict__ running_var) {
    __shared__ float run[BS_RUNS][BS_COLS];
    const int c = blockIdx.x * BS_COLS + threadIdx.x % BS_COLS;
    const float s = block_order_sum(part, blocks, C, c, run);
    if (threadIdx.x >= BS_COLS || c >= Cp) return;
    const float var = s / (float)M;
    rstd[c] = 1.0f / sqrtf(var + eps);
    if (running_mean) {
        running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean[c];
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (var * ((float)M / (float)(M - 1)));
    }
}

// where the 8 channels of row r begin in y's layout; step() moves on by the rpi rows between two rows of a thread
struct RowAt {
    long n;
    int t, L, dq, dr;
    __device__ __forceinline__ RowAt(long r, int L_, int rpi) : L(L_) {
        n = r / L;
        t = (int)(r - n * L);
        dq = rpi / L;
        dr = rpi - dq * L;
    }
    __device__ __forceinline__ long at(const BnArgs& p, int c0) const { return n * p.os_n + (long)t * p.os_t + c0; }
    __device__ __forceinline__ void step() {
        n += dq;
        t += dr;
        if (t >= L) { t -= L; ++n; }
    }
};

__global__ __launch_bounds__(BN_THREADS) void bn_normalise_kernel(BnArgs p) {
    const BnThread t(p.M, p.rows, p.C);
    const half_t* __restrict__ z = p.z;
    half_t* __restrict__ y = p.out;
    float mean[8], rstd[8], gamma[8], beta[8];
    load8(mean, p.mean, t.c0, p.Cp, 0.0f, 0.0f);
    load8(rstd, p.rstd, t.c0, p.Cp, 0.0f, 0.0f);
    load8(gamma, p.gamma, t.c0, p.Cp, 1.0f, 0.0f);
    load8(beta, p.beta, t.c0, p.Cp, 0.0f, 0.0f);
    RowAt at(t.first, p.L, t.rpi);
#pragma unroll 4
    for (long r = t.first; r < t.r_hi; r += t.rpi, at.step()) {
        const half8_t v = *(const half8_t*)(z + r * p.C + t.c0);
        half8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float u = fmaf(gamma[j], ((float)v[j] - mean[j]) * rstd[j], beta[j]);
            const float a = apply_act_rt(u, p.act);
            o[j] = t.c0 + j < p.Cp ? (half_t)fminf(fmaxf(a, p.lo), p.hi) : (half_t)0.0f;
        }
        *(half8_t*)(y + at.at(p, t.c0)) = o;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
// xh and du = dy [lo < y < hi] act'(gamma xh + beta) of one element
__device__ __forceinline__ float bn_du(float z, float dy, float yv, float mean, float rstd, float gamma, float beta, const BnArgs& p, float& xh) {
    xh = (z - mean) * rstd;
    const bool in = !p.clamped || (yv > p.lo && yv < p.hi);
    return in ? dy * act_grad(fmaf(gamma, xh, beta), p.act) : 0.0f;
}

// pass A: part[0][block][c] = sum du, part[1][block][c] = sum du xh over the block's rows
__global__ __launch_bounds__(BN_THREADS) void bn_grad_sums_kernel(BnArgs p) {
    __shared__ float red[BN_THREADS * 8];
    const BnThread t(p.M, p.rows, p.C);
    const half_t* __restrict__ z = p.z;
    float mean[8], rstd[8], gamma[8], beta[8];
    load8(mean, p.mean, t.c0, p.Cp, 0.0f, 0.0f);
    load8(rstd, p.rstd, t.c0, p.Cp, 0.0f, 0.0f);
    load8(gamma, p.gamma, t.c0, p.Cp, 1.0f, 0.0f);
    load8(beta, p.beta, t.c0, p.Cp, 0.0f, 0.0f);
    float sb[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, sg[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    RowAt at(t.first, p.L, t.rpi);
#pragma unroll 2
    for (long r = t.first; r < t.r_hi; r += t.rpi, at.step()) {
        const long a = at.at(p, t.c0);
        const half8_t v = *(const half8_t*)(z + r * p.C + t.c0);
        const half8_t d = *(const half8_t*)(p.dy + a);
        half8_t yv = {0, 0, 0, 0, 0, 0, 0, 0};
        if (p.clamped) yv = *(const half8_t*)(p.y + a);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float xh;
            const float du = bn_du((float)v[j], (float)d[j], (float)yv[j], mean[j], rstd[j], gamma[j], beta[j], p, xh);
            sb[j] += du;
            sg[j] = fmaf(du, xh, sg[j]);
        }
    }
    fold_slots(red, sb, t, p.C, p.part + (long)blockIdx.x * p.C);
    fold_slots(red, sg, t, p.C, p.part + (p.blocks + blockIdx.x) * p.C);
}

// sums[0][c] = dbeta, sums[1][c] = dgamma: the blocks' sums in block order; to dbeta / dgamma where they are asked for
__global__ __launch_bounds__(BS_COLS * BS_RUNS) void bn_grad_finish_kernel(const float* __restrict__ part, long blocks, int C, int Cp,
                                                                            float* __restrict__ sums, float* __restrict__ dgamma,
                                                                            float* __restrict__ dbeta) {
    __shared__ float run[BS_RUNS][BS_COLS];
    const int c = blockIdx.x * BS_COLS + threadIdx.x % BS_COLS;
    const float sb = block_order_sum(part, blocks, C, c, run);
    const float sg = block_order_sum(part + blocks * C, blocks, C, c, run);
    if (threadIdx.x >= BS_COLS || c >= C) return;
    sums[c] = sb;
    sums[C + c] = sg;
    if (c < Cp) {
        if (dbeta) dbeta[c] = sb;
        if (dgamma) dgamma[c] = sg;
    }
}

// pass B: dz = gamma rstd (du - dbeta / M - xh dgamma / M)
__global__ __launch_bounds__(BN_THREADS) void bn_dz_kernel(BnArgs p) {
    const BnThread t(p.M, p.rows, p.C);
    const half_t* __restrict__ z = p.z;
    half_t* __restrict__ dz = p.out;
    float mean[8], rstd[8], gamma[8], beta[8], mb[8], mg[8];
    load8(mean, p.mean, t.c0, p.Cp, 0.0f, 0.0f);
    load8(rstd, p.rstd, t.c0, p.Cp, 0.0f, 0.0f);
    load8(gamma, p.gamma, t.c0, p.Cp, 1.0f, 0.0f);
    load8(beta, p.beta, t.c0, p.Cp, 0.0f, 0.0f);
    const float inv_m = 1.0f / (float)p.M;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mb[j] = p.sums[t.c0 + j] * inv_m;
        mg[j] = p.sums[p.C + t.c0 + j] * inv_m;
    }
    RowAt at(t.first, p.L, t.rpi);
#pragma unroll 2
    for (long r = t.first; r < t.r_hi; r += t.rpi, at.step()) {
        const long a = at.at(p, t.c0);
        const half8_t v = *(const half8_t*)(z + r * p.C + t.c0);
        const half8_t d = *(const half8_t*)(p.dy + a);
        half8_t yv = {0, 0, 0, 0, 0, 0, 0, 0}, o;
        if (p.clamped) yv = *(const half8_t*)(p.y + a);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float xh;
            const float du = bn_du((float)v[j], (float)d[j], (float)yv[j], mean[j], rstd[j], gamma[j], beta[j], p, xh);
            o[j] = t.c0 + j < p.Cp ? (half_t)(gamma[j] * rstd[j] * (du - mb[j] - xh * mg[j])) : (half_t)0.0f;
        }
        *(half8_t*)(dz + r * p.C + t.c0) = o;
    }
}

}  // namespace
}  // namespace bh

size_t bh_k_batchnorm_train_workspace(int N, int L, int C) {
    return bh::bn_shape_error(N, L, C, C) ? 0 : bh::BnLayout((long)N * L, C).total;
}

#define BATCHNORM_TRAIN_CHECKS(what)                                                                                                         \
    const char* shape_err = bn_shape_error(N, L, C, C_param);                                                                                \
    BH_REQUIRE(!shape_err, what ": %s (N=%d L=%d C=%d C_param=%d)", shape_err, N, L, C, C_param);                                          \
    BH_REQUIRE(act_ok(act), what ": unknown activation %d", act);                                                                            \
    BH_REQUIRE(clamp_lo <= clamp_hi, what ": clamp range [%g, %g] is empty", (double)clamp_lo, (double)clamp_hi);                            \
    BH_REQUIRE(os_n >= 0 && os_t >= 0 && os_n % 8 == 0 && os_t % 8 == 0, what ": output strides must be multiples of 8");                   \
    BH_REQUIRE((gamma == nullptr) == (beta == nullptr), what ": gamma and beta come together or not at all (affine)");                       \
    const long M = (long)N * L;                                                                                                              \
    const BnLayout lay(M, C);                                                                                                                \
    BH_REQUIRE(workspace_bytes >= lay.total, what ": workspace of %zu bytes, bh_batchnorm_train_workspace = %zu", workspace_bytes, lay.total)

int bh_k_batchnorm_train_forward(const void* z, const float* gamma, const float* beta, float* running_mean, float* running_var, int N, int L,
                                 int C, int C_param, float eps, float momentum, int act, float clamp_lo, float clamp_hi, long os_n, long os_t,
                                 void* y, float* mean, float* rstd, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    using namespace bh;
    BATCHNORM_TRAIN_CHECKS("batchnorm_train_forward");
    BH_REQUIRE(eps > 0.0f && std::isfinite(eps), "batchnorm_train_forward: eps must be finite and > 0 (got %g)", (double)eps);
    BH_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "batchnorm_train_forward: momentum must be in 0..1 (got %g)", (double)momentum);
    BH_REQUIRE((running_mean == nullptr) == (running_var == nullptr),
               "batchnorm_train_forward: running_mean and running_var come together or not at all (track_running_stats)");
    BH_REQUIRE(z && y && mean && rstd && workspace, "batchnorm_train_forward: null pointer");
    BH_REQUIRE(aligned16(z) && aligned16(y) && aligned16(workspace), "batchnorm_train_forward: z, y and workspace must be 16-byte aligned");
    float* part = (float*)((char*)workspace + lay.part);
    const BnArgs a{(const half_t*)z, nullptr, nullptr, (half_t*)y, gamma, beta, mean, rstd, nullptr, part, M, bn_block_rows(M), lay.blocks, os_n,
                   os_t, L, C, C_param, act, is_clamped(clamp_lo, clamp_hi) ? 1 : 0, clamp_lo, clamp_hi};
    const dim3 grid((unsigned)lay.blocks), cols((C + BS_COLS - 1) / BS_COLS);
    hipLaunchKernelGGL(bn_sum_kernel, grid, dim3(BN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(bn_mean_kernel, cols, dim3(BS_COLS * BS_RUNS), 0, stream, (const float*)part, lay.blocks, C, C_param, M, mean);
    hipLaunchKernelGGL(bn_centred_kernel, grid, dim3(BN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(bn_rstd_kernel, cols, dim3(BS_COLS * BS_RUNS), 0, stream, (const float*)part, lay.blocks, C, C_param, M, eps, momentum,
                       (const float*)mean, rstd, running_mean, running_var);
    hipLaunchKernelGGL(bn_normalise_kernel, grid, dim3(BN_THREADS), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

int bh_k_batchnorm_train_backward(const void* z, const float* gamma, const float* beta, const float* mean, const float* rstd, const void* y,
                                  const void* dy, int N, int L, int C, int C_param, int act, float clamp_lo, float clamp_hi, long os_n, long os_t,
                                  void* dz, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    using namespace bh;
    BATCHNORM_TRAIN_CHECKS("batchnorm_train_backward");
    BH_REQUIRE(z && mean && rstd && y && dy && dz && workspace, "batchnorm_train_backward: null pointer");
    BH_REQUIRE(aligned16(z) && aligned16(y) && aligned16(dy) && aligned16(dz) && aligned16(workspace),
               "batchnorm_train_backward: z, y, dy, dz and workspace must be 16-byte aligned");
    float* part = (float*)((char*)workspace + lay.part);
    float* sums = (float*)((char*)workspace + lay.sums);
    const BnArgs a{(const half_t*)z, (const half_t*)y, (const half_t*)dy, (half_t*)dz, gamma, beta, mean, rstd, sums, part, M, bn_block_rows(M),
                   lay.blocks, os_n, os_t, L, C, C_param, act, is_clamped(clamp_lo, clamp_hi) ? 1 : 0, clamp_lo, clamp_hi};
    const dim3 grid((unsigned)lay.blocks), cols((C + BS_COLS - 1) / BS_COLS);
    hipLaunchKernelGGL(bn_grad_sums_kernel, grid, dim3(BN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(bn_grad_finish_kernel, cols, dim3(BS_COLS * BS_RUNS), 0, stream, (const float*)part, lay.blocks, C, C_param, sums, dgamma,
                       dbeta);
    hipLaunchKernelGGL(bn_dz_kernel, grid, dim3(BN_THREADS), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
