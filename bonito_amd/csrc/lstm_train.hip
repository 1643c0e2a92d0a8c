// One LSTM layer for TRAINING on gfx950: the forward that keeps what the backward needs, and the backward (dx, dW_ih, dW_hh, db).
// The layer is torch.nn.LSTM, one layer, one direction, as the reference wraps it (bonito/nn.py:353-397): gate order i, f, g, o,
// h_0 = c_0 = 0, insize == size == H, `reverse` runs the time loop backwards.
//     a_t = x_t W_ih^T + h_{t-1} W_hh^T + b       c_t = sig(f) c_{t-1} + sig(i) tanh(g)       h_t = sig(o) tanh(c_t)
// and, from the last processed step to the first,
//     d_t  = dh_t + da_{t+1} W_hh                  dc_t = dc_{t+1} sig(f_{t+1}) + d_t sig(o) (1 - tanh^2 c_t)
//     da_t = (dc_t tanh(g) sig'(i), dc_t c_{t-1} sig'(f), dc_t sig(i) (1 - tanh^2 g), d_t tanh(c_t) sig'(o))
//     dx_t = da_t W_ih      dW_ih = sum_t da_t^T x_t      dW_hh = sum_t da_t^T h_{t-1}      db = sum_{t,n} da_t
// Precision is that of autocast training: x, h, dh, dx fp16; the weights arrive as fp32 DEVICE tensors (the optimiser rewrites them
// every step) and the kernels use their round-to-nearest fp16 values; every sum is fp32; c is fp32 from step to step and where it is
// saved; dW_ih, dW_hh, db are fp32. The cell is LstmCell of lstm_cell.h, the one the inference kernels of lstm.hip call, so h has the
// bits they would publish from the same pre-activations, and the stored gates come from the cell's own exponentials.
//
// What is stored between the passes, all in buffers of the caller:
//     saved     : G [T][N][4H] fp16 - first x W_ih^T + b (bh_k_linear), then overwritten IN PLACE by the recurrent kernel with the
//                 post-activation gates sig(i), sig(f), tanh(g), sig(o);  c [T][N][H] fp32;  the fp16 copies of both weight matrices;
//                 h of the last two steps in fragment order (scratch of the forward)
//     workspace : da [T][N][4H] fp16;  dc_{t+1} sig(f_{t+1}) [N up to 16][H] fp32;  W_ih^T and W_hh in the backward's forms, fp16;  da of the
//                 last two steps in fragment order;  the partial sums of the weight gradients
//
// The two recurrences are the only serial work. A workgroup owns a tile of 16 chunks for all T steps; its waves split the H / 16 tiles
// of 16 units, each tile four gates x H / 32 (forward) or 4H / 32 (backward) v_mfma_f32_16x16x32_f16 with the 16 chunks as rows. The
// fp16 weights are re-read from L2 every step (1.18 MB at H = 384: no LDS holds them); the A operand - h_{t-1}, or da_{t+1} - is read
// back from a two-step buffer that the workgroup itself wrote one step earlier (in fragment order, see frag_index), behind ONE workgroup
// barrier per step. Batch tiles are independent:
// NO exchange between workgroups, no flags, no spin-waits - the kernels cannot hang, and any number of tiles fits one launch. Rows of a
// padded tile (chunk >= N) are taken as zeros and never stored, so they reach neither dx nor the weight gradients.
// Everything parallel over time is a GEMM over the T N rows: the input projection and dx = dA W_ih through bh_k_linear (linear_rows);
// dW = dA^T [X | H_prev] and db through reduce_rows, the reduction over rows every training layer shares (train_common.hip, row rule
// ROWS_LSTM): partial sums over blocks of rows that a second kernel adds IN A FIXED ORDER - no floating-point atomics, the results are
// byte-identical from call to call. The kernels of this file index with 64 bits throughout.
// Gradients are not clamped: da is stored as fp16 as autocast stores it, a |da| above 65504 becomes inf (loss scaling is the
// trainer's business), and a non-finite dh makes its chunk's dx and the weight gradients non-finite while the other chunks keep their bytes.
#include "lstm_cell.h"
#include "train_common.h"

namespace bh {
namespace {

constexpr int TILE_N = 16;             // chunks per workgroup of the recurrent kernels

inline bool shape_ok(int T, int N, int H) { return T >= 1 && N >= 1 && (long)T * N < (1l << 29) && H >= 32 && H <= 1024 && H % 32 == 0; }

struct SavedLayout {
    size_t gates, c, wih, whh, hfrag, total;
    SavedLayout(int T, int N, int H) {
        const size_t rows = (size_t)T * N, npad = (size_t)(N + TILE_N - 1) / TILE_N * TILE_N;
        gates = 0;
        c = align_up256(gates + rows * 4 * H * sizeof(half_t));
        wih = align_up256(c + rows * H * sizeof(float));
        whh = align_up256(wih + (size_t)4 * H * H * sizeof(half_t));
        hfrag = align_up256(whh + (size_t)4 * H * H * sizeof(half_t));         // [tiles][2][16 x H]: h of the last two steps, fragment order
        total = align_up256(hfrag + 2 * npad * H * sizeof(half_t));
    }
};

struct WorkLayout {
    size_t da, carry, wihT, whhT, dafrag, dw_part, db_part, total;
    WorkLayout(int T, int N, int H) {
        const size_t rows = (size_t)T * N;
        const Split g((long)T * N, 4 * H, 2 * H);        // the rows of dW = dA^T [X | H_prev]
        const size_t npad = (size_t)(N + TILE_N - 1) / TILE_N * TILE_N;
        da = 0;
        carry = align_up256(da + rows * 4 * H * sizeof(half_t));
        wihT = align_up256(carry + npad * H * sizeof(float));
        whhT = align_up256(wihT + (size_t)4 * H * H * sizeof(half_t));
        dafrag = align_up256(whhT + (size_t)4 * H * H * sizeof(half_t));       // [tiles][2][16 x 4H]: da of the last two steps, fragment order
        dw_part = align_up256(dafrag + 2 * npad * 4 * H * sizeof(half_t));
        db_part = align_up256(dw_part + (size_t)g.dw_splits * 4 * H * 2 * H * sizeof(float));
        total = align_up256(db_part + (size_t)g.db_splits * 4 * H * sizeof(float));
    }
};

// FRAGMENT ORDER. A wave reads an MFMA operand as 64 x 16 bytes, lane l = 8 halves of row (l & 15) at k = (l >> 4) * 8. From a
// row-major matrix that is 16 rows x 64 bytes, and the texture path takes the 16 rows one by one; so what the recurrences read every
// step is stored k-step by k-step as [k / 32][lane][8 halves], 1 KiB that the 64 lanes read as one contiguous piece:
__host__ __device__ __forceinline__ long frag_index(int row16, int k) {       // within one 16-row operand
    return ((long)(k >> 5) * 64 + ((k & 31) >> 3) * 16 + row16) * 8 + (k & 7);
}
enum WeightForm : int {
    W_ROWS = 0,      // [4H][H]: the W operand of bh_k_linear
    W_COLS = 1,      // transposed [H][4H]: the W operand of dx = dA W_ih
    W_FWD = 2,       // [H / 16 tiles][4 gates] operands of 16 units x H: B of h_{t-1} W_hh^T
    W_BWD = 3        // [H / 16 tiles] operands of 16 units x 4H: B of da_{t+1} W_hh
};
// fp32 [4H][H] -> its round-to-nearest fp16 values in one of the forms above
__global__ __launch_bounds__(256) void lstm_train_weights_kernel(const float* __restrict__ w, half_t* __restrict__ out, int form, int H) {
    const long total = 4l * H * H;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int r = (int)(e / H), c = (int)(e - (long)r * H);
        long at = e;
        if (form == W_COLS) at = (long)c * 4 * H + r;
        else if (form == W_FWD) at = ((long)(r % H >> 4) * 4 + r / H) * 16 * H + frag_index(r % H & 15, c);
        else if (form == W_BWD) at = (long)(c >> 4) * 16 * 4 * H + frag_index(c & 15, r);
        out[at] = (half_t)w[e];
    }
}

struct FwdArgs {
    const half_t* whh;      // fp16, W_FWD
    half_t* hfrag;          // [tiles][2][16 x H]: h_t of the tile in fragment order, by the parity of the step
    half_t* gates;          // [T][N][4H]: x W_ih^T + b on entry, the post-activation gates on exit
    float* c;               // [T][N][H]
    half_t* h;              // [T][N][H]
    int T, N, H, reverse;
};

// The K loop of both recurrences: acc[g] += A[16 chunks][K] x B_g[K][16 units], both operands in fragment order (`a`, `b` point at this
// lane's 8 halves of k-step 0, a k-step is 512 halves on, B_g starts g * bstep on). KU k-steps are loaded before their MFMAs are
// issued, so a wave keeps KU * (1 + NG) 16-byte loads in flight: the weights come from L2 every step, and it is the number of loads in
// flight that pays for their latency. The MFMAs are issued in ascending k whatever KU is. live = false (a padded chunk): the row is
// taken as zeros, whatever the buffer holds.
template <int NG, int KU>
__device__ __forceinline__ void k_loop(float4_t (&acc)[NG], const half_t* a, bool live, const half_t* b, long bstep, int ksteps) {
    const half8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
    int k = 0;
#pragma unroll 1
    for (; k + KU <= ksteps; k += KU) {
        half8_t fa[KU], fb[KU][NG];
#pragma unroll
        for (int j = 0; j < KU; ++j) {
            fa[j] = *(const half8_alias_t*)(a + (long)(k + j) * 512);
#pragma unroll
            for (int g = 0; g < NG; ++g) fb[j][g] = *(const half8_t*)(b + g * bstep + (long)(k + j) * 512);
        }
#pragma unroll
        for (int j = 0; j < KU; ++j)
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = mfma16(live ? fa[j] : zero, fb[j][g], acc[g]);
    }
#pragma unroll 1
    for (; k < ksteps; ++k) {
        const half8_t fa = *(const half8_alias_t*)(a + (long)k * 512);
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = mfma16(live ? fa : zero, *(const half8_t*)(b + g * bstep + (long)k * 512), acc[g]);
    }
}

__global__ __launch_bounds__(512) void lstm_train_fwd_kernel(FwdArgs p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int H = p.H, N = p.N, T = p.T;
    const int n0 = blockIdx.x * TILE_N, col = lane & 15, kg = lane >> 4;
    const bool live = n0 + col < N;                                         // the A row of this lane is a chunk of the batch
    half_t* hfrag = p.hfrag + (long)blockIdx.x * 2 * TILE_N * H;
    for (int s = 0; s < T; ++s) {
        const int t = p.reverse ? T - 1 - s : s, tp = p.reverse ? t + 1 : t - 1;
        const half_t* hprev = hfrag + (long)((s & 1) ^ 1) * TILE_N * H;     // written one step ago, behind the barrier
        half_alias_t* hnext = (half_alias_t*)hfrag + (long)(s & 1) * TILE_N * H;
        for (int tile = wave; tile < H / 16; tile += nw) {
            const int u = tile * 16 + col;
            // what the cell needs beside the sums, requested in front of the K loop: the projected gates and this thread's own c of the step before
            half_t gin[4][4];
            float cin[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + kg * 4 + i < N ? n0 + kg * 4 + i : N - 1;
                const half_alias_t* G = (const half_alias_t*)p.gates + ((long)t * N + n) * 4 * H + u;
#pragma unroll
                for (int g = 0; g < 4; ++g) gin[g][i] = G[g * H];
                cin[i] = s > 0 ? p.c[((long)tp * N + n) * H + u] : 0.0f;
            }
            float4_t acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
            if (s > 0)                                                      // h_0 = 0
                k_loop<4, 4>(acc, hprev + lane * 8, live, p.whh + (long)tile * 4 * 16 * H + lane * 8, 16l * H, H / 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + kg * 4 + i;
                if (n < N) {
                    const long row = (long)t * N + n;
                    half_alias_t* G = (half_alias_t*)p.gates + row * 4 * H + u;
                    const float ai = acc[0][i] + (float)gin[0][i], af = acc[1][i] + (float)gin[1][i];
                    const float ag = acc[2][i] + (float)gin[2][i], ao = acc[3][i] + (float)gin[3][i];
                    float c = cin[i];
                    const LstmCell cell(ai, af, ag, ao, c);
                    // the gates one by one, for the backward
                    G[0] = (half_t)cell.sig_i();
                    G[H] = (half_t)cell.sig_f();
                    G[2 * H] = (half_t)cell.tanh_g();
                    G[3 * H] = (half_t)cell.sig_o();
                    p.c[row * H + u] = c;
                    ((half_alias_t*)p.h)[row * H + u] = (half_t)cell.h;
                    hnext[frag_index(kg * 4 + i, u)] = (half_t)cell.h;
                }
            }
        }
        __syncthreads();                                                    // h_t of the whole tile is visible to the workgroup
    }
}

struct BwdArgs {
    const half_t* whhT;     // fp16, W_BWD
    half_t* dafrag;         // [tiles][2][16 x 4H]: da_t of the tile in fragment order, by the parity of the step
    const half_t* gates;    // post-activation [T][N][4H]
    const float* c;         // [T][N][H]
    const half_t* dh;       // [T][N][H]
    half_t* da;             // [T][N][4H]
    float* carry;           // [tiles x 16][H]: dc_{t+1} sig(f_{t+1})
    int T, N, H, reverse;
};

__global__ __launch_bounds__(512) void lstm_train_bwd_kernel(BwdArgs p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int H = p.H, N = p.N, T = p.T;
    const int n0 = blockIdx.x * TILE_N, col = lane & 15, kg = lane >> 4;
    const bool live = n0 + col < N;
    half_t* dafrag = p.dafrag + (long)blockIdx.x * 2 * TILE_N * 4 * H;
    for (int s = T - 1; s >= 0; --s) {
        const int t = p.reverse ? T - 1 - s : s;
        const int tp = p.reverse ? t + 1 : t - 1;                           // the step processed before t (s > 0)
        const half_t* danext = dafrag + (long)((s & 1) ^ 1) * TILE_N * 4 * H;     // written one iteration ago, behind the barrier
        half_alias_t* dathis = (half_alias_t*)dafrag + (long)(s & 1) * TILE_N * 4 * H;
        for (int tile = wave; tile < H / 16; tile += nw) {
            const int u = tile * 16 + col;
            half_t gin[4][4], dhin[4];
            float ct[4], cp[4], cy[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + kg * 4 + i < N ? n0 + kg * 4 + i : N - 1;
                const long row = (long)t * N + n;
#pragma unroll
                for (int g = 0; g < 4; ++g) gin[g][i] = p.gates[row * 4 * H + g * H + u];
                dhin[i] = p.dh[row * H + u];
                ct[i] = p.c[row * H + u];
                cp[i] = s > 0 ? p.c[((long)tp * N + n) * H + u] : 0.0f;
                cy[i] = s < T - 1 ? p.carry[(long)(n0 + kg * 4 + i) * H + u] : 0.0f;     // this thread's own store of the step before
            }
            float4_t acc[1] = {float4_t{0.0f, 0.0f, 0.0f, 0.0f}};
            if (s < T - 1)
                k_loop<1, 8>(acc, danext + lane * 8, live, p.whhT + (long)tile * 16 * 4 * H + lane * 8, 0, 4 * H / 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + kg * 4 + i;
                if (n < N) {
                    const long row = (long)t * N + n;
                    const float si = (float)gin[0][i], sf = (float)gin[1][i], tg = (float)gin[2][i], so = (float)gin[3][i];
                    const float ec = __expf(-2.0f * __builtin_amdgcn_fmed3f(ct[i], -12.5f, 12.5f));
                    const float tc = __fmul_rn(1.0f - ec, rcpf_(1.0f + ec));
                    const float d = acc[0][i] + (float)dhin[i];
                    const float dc = d * so * (1.0f - tc * tc) + cy[i];
                    p.carry[(long)n * H + u] = dc * sf;
                    half_alias_t* da = (half_alias_t*)p.da + row * 4 * H + u;
                    const half_t dg[4] = {(half_t)(dc * tg * si * (1.0f - si)), (half_t)(dc * cp[i] * sf * (1.0f - sf)),
                                          (half_t)(dc * si * (1.0f - tg * tg)), (half_t)(d * tc * so * (1.0f - so))};
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        da[g * H] = dg[g];
                        dathis[frag_index(kg * 4 + i, g * H + u)] = dg[g];
                    }
                }
            }
        }
        __syncthreads();                                                    // da_t of the whole tile is visible to the workgroup
    }
}

inline int recurrent_threads(int H) {
    const int tiles = H / 16;
    return 64 * (tiles < 8 ? tiles : 8);
}

}  // namespace
}  // namespace bh

size_t bh_k_lstm_train_saved_bytes(int T, int N, int H) { return bh::shape_ok(T, N, H) ? bh::SavedLayout(T, N, H).total : 0; }
size_t bh_k_lstm_train_backward_workspace(int T, int N, int H) { return bh::shape_ok(T, N, H) ? bh::WorkLayout(T, N, H).total : 0; }
int bh_k_lstm_train_workgroups(int N) { return N >= 1 ? (N + bh::TILE_N - 1) / bh::TILE_N : 0; }

#define LSTM_TRAIN_SHAPE(what)                                                                                                    \
    BH_REQUIRE(T >= 1 && N >= 1, what ": T and N must be positive (got T=%d N=%d)", T, N);                                        \
    BH_REQUIRE(H >= 32 && H <= 1024 && H % 32 == 0, what ": hidden size %d is not supported (a multiple of 32 in 32..1024)", H);  \
    BH_REQUIRE((long)T * N < (1l << 29), what ": T * N = %ld rows are too many for one call (below 2^29)", (long)T * N)

int bh_k_lstm_train_forward(const void* x, const float* w_ih, const float* w_hh, const float* bias, int T, int N, int H, int reverse,
                            void* h_out, void* saved, size_t saved_bytes, hipStream_t stream) {
    using namespace bh;
    LSTM_TRAIN_SHAPE("lstm_train_forward");
    BH_REQUIRE(x && w_ih && w_hh && h_out && saved, "lstm_train_forward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(h_out) && aligned16(saved), "lstm_train_forward: x, h_out and saved must be 16-byte aligned");
    BH_REQUIRE(reverse == 0 || reverse == 1, "lstm_train_forward: reverse must be 0 or 1 (got %d)", reverse);
    const SavedLayout L(T, N, H);
    BH_REQUIRE(saved_bytes >= L.total, "lstm_train_forward: saved buffer of %zu bytes, bh_lstm_train_saved_bytes(%d, %d, %d) = %zu", saved_bytes,
               T, N, H, L.total);
    char* sv = (char*)saved;
    half_t* wih16 = (half_t*)(sv + L.wih);
    half_t* whh16 = (half_t*)(sv + L.whh);
    const int grid = cvt_grid(4l * H * H);
    hipLaunchKernelGGL(lstm_train_weights_kernel, dim3(grid), dim3(256), 0, stream, w_ih, wih16, (int)W_ROWS, H);
    hipLaunchKernelGGL(lstm_train_weights_kernel, dim3(grid), dim3(256), 0, stream, w_hh, whh16, (int)W_FWD, H);
    BH_CHECK_HIP(hipGetLastError());
    // G = x W_ih^T + b over all T N rows, fp16
    if (int rc = linear_rows((const half_t*)x, wih16, bias, (half_t*)(sv + L.gates), T, N, H, 4 * H, ACT_NONE, 1.0f, -INFINITY, INFINITY, false, false, stream))
        return rc;
    FwdArgs a{whh16, (half_t*)(sv + L.hfrag), (half_t*)(sv + L.gates), (float*)(sv + L.c), (half_t*)h_out, T, N, H, reverse};
    hipLaunchKernelGGL(lstm_train_fwd_kernel, dim3((N + TILE_N - 1) / TILE_N), dim3(recurrent_threads(H)), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

int bh_k_lstm_train_backward(const void* x, const float* w_ih, const float* w_hh, const void* h, const void* saved, const void* dh, int T,
                             int N, int H, int reverse, void* dx, float* dw_ih, float* dw_hh, float* dbias, void* workspace,
                             size_t workspace_bytes, hipStream_t stream) {
    using namespace bh;
    LSTM_TRAIN_SHAPE("lstm_train_backward");
    BH_REQUIRE(x && w_ih && w_hh && h && saved && dh && dx && dw_ih && dw_hh && workspace, "lstm_train_backward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(h) && aligned16(saved) && aligned16(dh) && aligned16(dx) && aligned16(workspace),
               "lstm_train_backward: x, h, saved, dh, dx and workspace must be 16-byte aligned");
    BH_REQUIRE(reverse == 0 || reverse == 1, "lstm_train_backward: reverse must be 0 or 1 (got %d)", reverse);
    const SavedLayout L(T, N, H);
    const WorkLayout W(T, N, H);
    BH_REQUIRE(workspace_bytes >= W.total, "lstm_train_backward: workspace of %zu bytes, bh_lstm_train_backward_workspace(%d, %d, %d) = %zu",
               workspace_bytes, T, N, H, W.total);
    const char* sv = (const char*)saved;
    char* ws = (char*)workspace;
    half_t* da = (half_t*)(ws + W.da);
    half_t* wihT = (half_t*)(ws + W.wihT);
    half_t* whhT = (half_t*)(ws + W.whhT);
    const int grid = cvt_grid(4l * H * H);
    hipLaunchKernelGGL(lstm_train_weights_kernel, dim3(grid), dim3(256), 0, stream, w_ih, wihT, (int)W_COLS, H);
    hipLaunchKernelGGL(lstm_train_weights_kernel, dim3(grid), dim3(256), 0, stream, w_hh, whhT, (int)W_BWD, H);
    BwdArgs a{whhT, (half_t*)(ws + W.dafrag), (const half_t*)(sv + L.gates), (const float*)(sv + L.c), (const half_t*)dh, da, (float*)(ws + W.carry), T, N, H, reverse};
    hipLaunchKernelGGL(lstm_train_bwd_kernel, dim3((N + TILE_N - 1) / TILE_N), dim3(recurrent_threads(H)), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    // dx = dA W_ih over all T N rows, fp16
    if (int rc = linear_rows(da, wihT, nullptr, (half_t*)dx, T, N, 4 * H, H, ACT_NONE, 1.0f, -INFINITY, INFINITY, false, false, stream)) return rc;
    // dW_ih, dW_hh = dA^T [X | H_prev] and db = the column sums of dA, over all T N rows
    const RowRule rule{(const half_t*)x, ROWS_LSTM, H, 0, 0, 0, 0, 0, (const half_t*)h, T, N, reverse};
    return reduce_rows(da, rule, (long)T * N, 4 * H, 2 * H, (float*)(ws + W.dw_part), (float*)(ws + W.db_part), dw_ih, dw_hh, dbias, stream);
}
