// The two layers a transformer encoder layer adds to training on gfx950: the backward of the DeepNorm residual RMSNorm, and the gated
// input layer of the MLP (fc1 + SwiGLU), forward and backward. With attention_train.hip and the linear layer of train_layers.hip this is
// every piece of a TransformerEncoderLayer (bonito_amd.attn.encoder_layer chains them). The arithmetic is stated in
// include/bonito_hip.h under bh_rmsnorm_train_backward.
//
// Norm. The forward is bh_k_rmsnorm_residual as it stands and saves nothing: the backward reads a and x anyway and recomputes
//     z = a + alpha x      r = rsqrt(mean_d z^2 + eps)
// then, with g = dy w and c = (1/D) sum_d g_d z_d:   dz = r g - r^3 c z,  da = fp16(dz),  dx = fp16(alpha dz),  dw_d = sum_m dy z r.
// One wave per row, up to two 16-byte vectors per lane (D <= 1024), as in the forward kernel. A workgroup of four waves owns a block
// of consecutive rows; a lane keeps the dw sums of its own columns in registers over the block's rows, the four waves are added in wave
// order through LDS, and a second launch adds the blocks in block order: no floating-point atomics, the split a function of (M, D).
//
// Gated layer. Forward: the rounded weights are written with rows interleaved (y_j, gate_j), the layout create_transformer (engine.cpp)
// uploads, and bh_k_linear runs with gated = 1 through linear_rows: h has the engine's bytes. Backward: u = x W1^T is recomputed by the
// plain GEMM in torch's row order [y | gate], gated_du_kernel turns it in place into du = [dy | dgate], then dx = du W1 through
// linear_rows on the transposed rounded weights and dW1 = du^T x through reduce_rows (train_common.hip).
// Every kernel of this file indexes with 64 bits.
#include <cmath>

#include "train_common.h"

namespace bh {
namespace {

// ---- norm ---------------------------------------------------------------------------------------------------------------------------------
constexpr int NORM_WAVES = 4;           // rows in flight per workgroup
constexpr int NORM_MAX_D = 1024;
constexpr long NORM_MIN_ROWS = 64;      // rows of a dw block, at least
constexpr long NORM_MAX_BLOCKS = 1024;

// rows per dw block: a function of M alone (a multiple of the four rows a workgroup has in flight)
inline long norm_block_rows(long M) {
    long rows = (M + NORM_MAX_BLOCKS - 1) / NORM_MAX_BLOCKS;
    if (rows < NORM_MIN_ROWS) rows = NORM_MIN_ROWS;
    return (rows + NORM_WAVES - 1) / NORM_WAVES * NORM_WAVES;
}
inline long norm_blocks(long M) { const long rows = norm_block_rows(M); return (M + rows - 1) / rows; }

const char* norm_shape_error(long M, int D) {
    if (M < 1 || M >= (1l << 40)) return "M must be in 1..2^40-1";
    if (D < 8 || D % 8 != 0 || D > NORM_MAX_D) return "D must be a multiple of 8 in 8..1024";
    return nullptr;
}

struct NormBwdArgs {
    const half_t* a;
    const half_t* x;
    const float* w;
    const half_t* dy;
    half_t* da;             // may be null
    half_t* dx;             // may be null
    float* part;            // [blocks][D]
    long M, rows;
    int D;
    float alpha, eps;
};

__global__ __launch_bounds__(64 * NORM_WAVES) void rmsnorm_bwd_kernel(NormBwdArgs p) {
    __shared__ float red[NORM_WAVES][NORM_MAX_D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r_lo = (long)blockIdx.x * p.rows, r_hi = r_lo + p.rows < p.M ? r_lo + p.rows : p.M;
    const int nv = p.D >> 3;
    const float inv_d = 1.0f / (float)p.D;
    float wv[2][8], dw[2][8];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int idx = lane + 64 * v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            wv[v][e] = idx < nv ? p.w[idx * 8 + e] : 0.0f;
            dw[v][e] = 0.0f;
        }
    }
    for (long row = r_lo + wave; row < r_hi; row += NORM_WAVES) {
        const long at = row * p.D;
        float z[2][8], g[2][8], d[2][8];
        float ss = 0.0f, gz = 0.0f;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int idx = lane + 64 * v;
            if (idx < nv) {
                const half8_t av = *(const half8_t*)(p.a + at + idx * 8);
                const half8_t xv = *(const half8_t*)(p.x + at + idx * 8);
                const half8_t dv = *(const half8_t*)(p.dy + at + idx * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    z[v][e] = (float)av[e] + p.alpha * (float)xv[e];
                    d[v][e] = (float)dv[e];
                    g[v][e] = d[v][e] * wv[v][e];
                    ss += z[v][e] * z[v][e];
                    gz += g[v][e] * z[v][e];
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            ss += __shfl_xor(ss, off);
            gz += __shfl_xor(gz, off);
        }
        const float r = rsqrtf(ss * inv_d + p.eps);
        const float k = r * r * r * (gz * inv_d);
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int idx = lane + 64 * v;
            if (idx < nv) {
                half8_t oa, ox;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float dz = r * g[v][e] - k * z[v][e];
                    oa[e] = (half_t)dz;
                    ox[e] = (half_t)(p.alpha * dz);
                    dw[v][e] += d[v][e] * z[v][e] * r;
                }
                if (p.da) *(half8_t*)(p.da + at + idx * 8) = oa;
                if (p.dx) *(half8_t*)(p.dx + at + idx * 8) = ox;
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int idx = lane + 64 * v;
        if (idx < nv) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[wave][idx * 8 + e] = dw[v][e];
        }
    }
    __syncthreads();
    float* out = p.part + (long)blockIdx.x * p.D;
    for (int c = threadIdx.x; c < p.D; c += 64 * NORM_WAVES) {
        float s = red[0][c];
#pragma unroll
        for (int q = 1; q < NORM_WAVES; ++q) s += red[q][c];
        out[c] = s;
    }
}

// dw[c] = the blocks' partial sums in block order (block_order_sum, train_common.h; one thread per column over all blocks is a chain of
// as many dependent loads: DESIGN.md section 6 has both times)
__global__ __launch_bounds__(BS_COLS * BS_RUNS) void rmsnorm_dw_kernel(const float* __restrict__ part, long blocks, int D, float* __restrict__ dw) {
    __shared__ float run[BS_RUNS][BS_COLS];
    const int c = blockIdx.x * BS_COLS + threadIdx.x % BS_COLS;
    const float s = block_order_sum(part, blocks, D, c, run);
    if (threadIdx.x < BS_COLS && c < D) dw[c] = s;
}

// ---- gated layer --------------------------------------------------------------------------------------------------------------------------
// in place over u [M][2F] = [y | gate]:  s = sigmoid(gate),  dy = dh gate s,  dgate = dh y s (1 + gate (1 - s));  u <- [dy | dgate]
__global__ __launch_bounds__(256) void gated_du_kernel(half_t* __restrict__ u, const half_t* __restrict__ dh, long M, int F) {
    const long fv = F / 8, total = M * fv;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long m = e / fv, j = (e - m * fv) * 8;
        half_t* yp = u + m * (2l * F) + j;
        half_t* gp = yp + F;
        const half8_t y8 = *(const half8_t*)yp, g8 = *(const half8_t*)gp, d8 = *(const half8_t*)(dh + m * (long)F + j);
        half8_t oy, og;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float y = (float)y8[i], gate = (float)g8[i], d = (float)d8[i];
            const float s = sigmoidf_(gate);
            oy[i] = (half_t)(d * gate * s);
            og[i] = (half_t)(d * y * s * (1.0f + gate * (1.0f - s)));
        }
        *(half8_t*)yp = oy;
        *(half8_t*)gp = og;
    }
}

struct GatedLayout {
    size_t w, u, dw_part, total;
    GatedLayout(long M, int D, int F) {
        const Split g(M, 2 * F, D);
        w = 0;                                  // forward: fp16 interleaved [2F][D]; backward: fp16 [2F][D], then [D][2F]
        u = align_up256(w + (size_t)2 * F * D * sizeof(half_t));
        dw_part = align_up256(u + (size_t)M * 2 * F * sizeof(half_t));
        total = align_up256(dw_part + (size_t)g.dw_splits * 2 * F * D * sizeof(float));
    }
};

const char* gated_shape_error(long M, int D, int F) {
    if (M < 1 || M >= (1l << 31)) return "M must be in 1..2^31-1";
    if (D < 8 || D % 8 != 0 || D > 16384) return "D must be a multiple of 8 up to 16384";
    if (F < 8 || F % 8 != 0 || F > 8192) return "F must be a multiple of 8 up to 8192";
    return nullptr;
}

}  // namespace
}  // namespace bh

size_t bh_k_rmsnorm_train_workspace(long M, int D) {
    return bh::norm_shape_error(M, D) ? 0 : bh::align_up256((size_t)bh::norm_blocks(M) * D * sizeof(float));
}

int bh_k_rmsnorm_train_backward(const void* a, const void* x, const float* w, const void* dy, long M, int D, float alpha, float eps, void* da,
                                void* dx, float* dw, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    using namespace bh;
    const char* shape_err = norm_shape_error(M, D);
    BH_REQUIRE(!shape_err, "rmsnorm_train_backward: %s (M=%ld D=%d)", shape_err, M, D);
    BH_REQUIRE(std::isfinite(alpha) && eps >= 0.0f && std::isfinite(eps), "rmsnorm_train_backward: alpha must be finite and eps >= 0");
    BH_REQUIRE(a && x && w && dy && dw && workspace, "rmsnorm_train_backward: null pointer");
    BH_REQUIRE(aligned16(a) && aligned16(x) && aligned16(dy) && aligned16(da) && aligned16(dx) && aligned16(workspace),
               "rmsnorm_train_backward: a, x, dy, da, dx and workspace must be 16-byte aligned");
    const size_t need = bh_k_rmsnorm_train_workspace(M, D);
    BH_REQUIRE(workspace_bytes >= need, "rmsnorm_train_backward: workspace of %zu bytes, bh_rmsnorm_train_workspace = %zu", workspace_bytes, need);
    const long blocks = norm_blocks(M);
    NormBwdArgs p{(const half_t*)a, (const half_t*)x, w, (const half_t*)dy, (half_t*)da, (half_t*)dx, (float*)workspace, M, norm_block_rows(M),
                  D, alpha, eps};
    hipLaunchKernelGGL(rmsnorm_bwd_kernel, dim3((unsigned)blocks), dim3(64 * NORM_WAVES), 0, stream, p);
    hipLaunchKernelGGL(rmsnorm_dw_kernel, dim3((D + BS_COLS - 1) / BS_COLS), dim3(BS_COLS * BS_RUNS), 0, stream, (const float*)workspace, blocks,
                       D, dw);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

size_t bh_k_gated_linear_train_workspace(long M, int D, int F) {
    return bh::gated_shape_error(M, D, F) ? 0 : bh::GatedLayout(M, D, F).total;
}

#define GATED_TRAIN_CHECKS(what)                                                                                               \
    const char* shape_err = gated_shape_error(M, D, F);                                                                       \
    BH_REQUIRE(!shape_err, what ": %s (M=%ld D=%d F=%d)", shape_err, M, D, F);                                               \
    const GatedLayout L(M, D, F);                                                                                             \
    BH_REQUIRE(workspace_bytes >= L.total, what ": workspace of %zu bytes, bh_gated_linear_train_workspace = %zu", workspace_bytes, L.total)

int bh_k_gated_linear_train_forward(const void* x, const float* w, long M, int D, int F, void* h, void* workspace, size_t workspace_bytes,
                                    hipStream_t stream) {
    using namespace bh;
    GATED_TRAIN_CHECKS("gated_linear_train_forward");
    BH_REQUIRE(x && w && h && workspace, "gated_linear_train_forward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(h) && aligned16(workspace), "gated_linear_train_forward: x, h and workspace must be 16-byte aligned");
    half_t* w16 = (half_t*)((char*)workspace + L.w);
    if (int rc = round_weights(w, w16, 2 * F, D, WEIGHTS_GATED_PAIRS, stream)) return rc;
    return linear_rows((const half_t*)x, w16, nullptr, (half_t*)h, (int)M, 1, D, 2 * F, ACT_NONE, 1.0f, -INFINITY, INFINITY, false, true, stream);
}

int bh_k_gated_linear_train_backward(const void* x, const float* w, const void* dh, long M, int D, int F, void* dx, float* dw, void* workspace,
                                     size_t workspace_bytes, hipStream_t stream) {
    using namespace bh;
    GATED_TRAIN_CHECKS("gated_linear_train_backward");
    BH_REQUIRE(x && w && dh && dw && workspace, "gated_linear_train_backward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(dh) && aligned16(dx) && aligned16(workspace),
               "gated_linear_train_backward: x, dh, dx and workspace must be 16-byte aligned");
    char* ws = (char*)workspace;
    half_t* w16 = (half_t*)(ws + L.w);
    half_t* u = (half_t*)(ws + L.u);
    // u = x W1^T in torch's row order, then du in place
    if (int rc = round_weights(w, w16, 2 * F, D, WEIGHTS_ROWS, stream)) return rc;
    if (int rc = linear_rows((const half_t*)x, w16, nullptr, u, (int)M, 1, D, 2 * F, ACT_NONE, 1.0f, -INFINITY, INFINITY, false, false, stream))
        return rc;
    const long items = M * (F / 8);
    hipLaunchKernelGGL(gated_du_kernel, dim3((unsigned)((items + 255) / 256 < 65536 ? (items + 255) / 256 : 65536)), dim3(256), 0, stream, u,
                       (const half_t*)dh, M, F);
    BH_CHECK_HIP(hipGetLastError());
    if (dx) {      // dx = du W1 over all rows, fp16
        if (int rc = round_weights(w, w16, 2 * F, D, WEIGHTS_TRANSPOSED, stream)) return rc;
        if (int rc = linear_rows(u, w16, nullptr, (half_t*)dx, (int)M, 1, 2 * F, D, ACT_NONE, 1.0f, -INFINITY, INFINITY, false, false, stream))
            return rc;
    }
    const RowRule rule{(const half_t*)x, ROWS_PLAIN, D};
    return reduce_rows(u, rule, M, 2 * F, D, (float*)(ws + L.dw_part), nullptr, dw, nullptr, nullptr, stream);
}
