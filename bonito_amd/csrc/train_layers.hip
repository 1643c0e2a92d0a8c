// The convolution and the linear / CRF-head layer for TRAINING on gfx950: a forward that rounds the fp32 master weights on the device
// and calls the inference kernels, and the backward (dx, dW, db). With lstm_train.hip and seqdist_grad.hip this is every layer of an
// LSTM-family CRF model (conv x3 -> LSTM x n -> [linear] -> linearcrfencoder), SeqdistModel.forward_train chains them.
//     convolution   y = clamp(act(conv(x, W) + b), lo, hi)          x [N][Lin][Cin] channel-minor ([N][Lin] for Cin == 1), y at n os_n + t os_t + c
//     linear        Y = clamp(act(X W^T + b) scale, lo, hi)         X [M][K], rows m = t N + n; Y [T][N][C] or batch-major [N][T][C]
// Precision is that of autocast training, as for the LSTM layer: activations and their gradients fp16; W and b arrive as fp32 DEVICE
// tensors (the optimiser rewrites them every step) and every kernel uses their round-to-nearest fp16 values; every sum is fp32; dW and
// db are fp32.
//
// Forward. The rounded weights are written in the layout the inference kernel reads (conv_pack_kernel: the bytes of bh_conv1d_pack;
// fp16 values held in fp32 for the Cin == 1 kernel and for every bias), then bh_k_conv_first / bh_k_conv_igemm / bh_k_linear run: y
// has the bytes the inference entry points produce from the same rounded weights.
//
// Backward, from dy in the layout of y:
//     dz = dy m act'(z)  (linear: dy m scale act'), stored fp16 in ROW order (conv: m = n Lout + t; linear: m = t N + n).
//     m = [lo < y < hi] is read from the STORED fp16 y - a recomputed y can land one ulp on the other side of a bound, and the clamp's
//     gradient is discontinuous. Convolution: act' at z recomputed in fp32 from x and the rounded weights (conv_dz_kernel, an implicit
//     GEMM on MFMA 16x16x32 whose both operands are 16-byte global loads: a window of the channel-minor x is contiguous; Cin == 1 on the
//     VALU). Linear: tanh' = 1 - (Y / scale)^2 from the stored Y.
//     dW = dz^T B over the M rows and db = sum of dz come from reduce_rows (train_common.hip), the reduction over rows of every
//     training layer: B's row m is X[m] for the linear layer (ROWS_PLAIN) and, for the convolution, the window of K Cin contiguous
//     halves at x[n][t s - p], zero where it hangs over an edge (ROWS_CONV). The rows are split into blocks whose partial sums are
//     added in block order: no floating-point atomics, equal bytes from call to call.
//     dx: linear through linear_rows on W^T (fp16 copy made by round_weights, train_common.hip); convolution in conv_dx_kernel, one thread per 8
//     input channels of one input position, taps with (l + p - k) mod s == 0 only, fp32 sums in a fixed order.
// Every kernel of this file indexes with 64 bits. bh_k_linear is called through linear_rows (train_common.hip), on blocks of rows whose
// operands stay below 2^30 halves.
#include <cmath>

#include "train_common.h"

namespace bh {
namespace {

inline int out_len(int Lin, int K, int stride, int pad) { return (Lin + 2 * pad - K) / stride + 1; }

// ---- the master weights, rounded, in the forms the kernels read ---------------------------------------------------------------------------
// fp32 [Cout][Cin][K] -> fp16 [Cout16][Kp], column k * Cin + c, zero elsewhere: the bytes of bh_conv1d_pack
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ w, half_t* __restrict__ out, int Cin, int Cout, int K, int Kp,
                                                        long total) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int f = (int)(e / Kp), kk = (int)(e - (long)f * Kp);
        half_t v = (half_t)0.0f;
        if (f < Cout && kk < K * Cin) {
            const int k = kk / Cin, c = kk - k * Cin;
            v = (half_t)w[((long)f * Cin + c) * K + k];
        }
        out[e] = v;
    }
}
// fp32 -> the fp16 value, held in fp32 (in == null: zeros)
__global__ __launch_bounds__(256) void round_kernel(const float* __restrict__ in, float* __restrict__ out, long n) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x)
        out[e] = in ? (float)(half_t)in[e] : 0.0f;
}

// ---- convolution: dz ----------------------------------------------------------------------------------------------------------------
struct ConvBwdArgs {
    const half_t* x;        // [N][Lin][Cin]
    const half_t* wpk;      // [Cout16][Kp] fp16 (Cin % 8 == 0)
    const float* w1;        // [Cout][K] rounded, fp32 (Cin == 1)
    const float* bias;      // [Cout] rounded, fp32
    const half_t* y;        // at n os_n + t os_t + c
    const half_t* dy;
    half_t* dz;             // [N][Lout][Cout]
    half_t* dx;             // [N][Lin][Cin]
    int N, Lin, Lout, Cin, Cout, K, stride, pad, act, Kp, clamped, tblocks;
    float lo, hi;
    long os_n, os_t;
};

// z of 64 positions x 64 features per workgroup: A = packed weight rows (features), B = the positions' windows, K loop over Kp / 32
// k-steps; a lane ends with 4 consecutive features of one position and finishes them: dz = dy [lo < y < hi] act'(z + b)
__global__ __launch_bounds__(256) void conv_dz_kernel(ConvBwdArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n = blockIdx.x / p.tblocks;
    const int t = (int)(blockIdx.x - n * p.tblocks) * 64 + wave * 16 + (lane & 15);
    const int f0 = blockIdx.y * 64, kg = lane >> 4;
    const bool live = t < p.Lout;
    const half_t* xn = p.x + n * p.Lin * p.Cin;
    const int KC = p.K * p.Cin, c16 = (p.Cout + 15) / 16 * 16;
    float4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
    for (int ks = 0; ks < p.Kp / 32; ++ks) {
        const int kk = ks * 32 + kg * 8;
        half8_t b = {0, 0, 0, 0, 0, 0, 0, 0};
        if (live && kk < KC) {
            const int k = kk / p.Cin, ci = kk - k * p.Cin;
            const int l = t * p.stride - p.pad + k;
            if (l >= 0 && l < p.Lin) b = *(const half8_t*)(xn + (long)l * p.Cin + ci);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (f0 + j * 16 < c16)
                acc[j] = mfma16(*(const half8_t*)(p.wpk + (long)(f0 + j * 16 + (lane & 15)) * p.Kp + kk), b, acc[j]);
    }
    if (!live) return;
    const long at = n * p.os_n + (long)t * p.os_t;
    half_t* dzr = p.dz + (n * p.Lout + t) * p.Cout;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = f0 + j * 16 + kg * 4;
        if (f >= p.Cout) continue;
        const half4_t dy4 = *(const half4_t*)(p.dy + at + f);
        half4_t y4 = {0, 0, 0, 0}, o;
        if (p.clamped) y4 = *(const half4_t*)(p.y + at + f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float yv = (float)y4[i];
            const bool in = !p.clamped || (yv > p.lo && yv < p.hi);
            o[i] = in ? (half_t)((float)dy4[i] * act_grad(acc[j][i] + p.bias[f + i], p.act)) : (half_t)0.0f;
        }
        *(half4_t*)(dzr + f) = o;
    }
}

// Cin == 1: one thread per output position, the taps in the order of conv_first_kernel
__global__ __launch_bounds__(256) void conv_first_dz_kernel(ConvBwdArgs p) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)p.N * p.Lout) return;
    const long n = e / p.Lout;
    const int t = (int)(e - n * p.Lout);
    const half_t* xn = p.x + n * p.Lin;
    float xw[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const int l = t * p.stride - p.pad + k;
        xw[k] = (k < p.K && l >= 0 && l < p.Lin) ? (float)xn[l] : 0.0f;
    }
    const long at = n * p.os_n + (long)t * p.os_t;
    half_t* dzr = p.dz + e * p.Cout;
    for (int c = 0; c < p.Cout; ++c) {
        float z = p.bias[c];
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (k < p.K) z = fmaf(p.w1[c * p.K + k], xw[k], z);
        const float yv = p.clamped ? (float)p.y[at + c] : 0.0f;
        const bool in = !p.clamped || (yv > p.lo && yv < p.hi);
        dzr[c] = in ? (half_t)((float)p.dy[at + c] * act_grad(z, p.act)) : (half_t)0.0f;
    }
}

// ---- convolution: dx ----------------------------------------------------------------------------------------------------------------
// dx[n][l][ci] = sum over the taps k with (l + p - k) mod s == 0, t = (l + p - k) / s in [0, Lout), and over co, of W[co][ci][k] dz[n][t][co]:
// one thread per 8 input channels of one input position, k ascending, co ascending, fp32
__global__ __launch_bounds__(256) void conv_dx_kernel(ConvBwdArgs p) {
    const int cv = p.Cin / 8;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)p.N * p.Lin * cv) return;
    const long nl = e / cv, n = nl / p.Lin;
    const int ci = (int)(e - nl * cv) * 8, l = (int)(nl - n * p.Lin);
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int q = l + p.pad;
    for (int k = q % p.stride; k < p.K && k <= q; k += p.stride) {
        const int t = (q - k) / p.stride;
        if (t >= p.Lout) continue;
        const half_t* dzr = p.dz + (n * p.Lout + t) * p.Cout;
        const half_t* wr = p.wpk + (long)k * p.Cin + ci;
        for (int co = 0; co < p.Cout; co += 4) {
            const half4_t d = *(const half4_t*)(dzr + co);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const half8_t w = *(const half8_t*)(wr + (long)(co + i) * p.Kp);
                const float g = (float)d[i];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = fmaf(g, (float)w[j], acc[j]);
            }
        }
    }
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)acc[j];
    *(half8_t*)(p.dx + nl * p.Cin + ci) = o;
}

// Cin == 1: one thread per input sample
__global__ __launch_bounds__(256) void conv_first_dx_kernel(ConvBwdArgs p) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)p.N * p.Lin) return;
    const long n = e / p.Lin;
    const int l = (int)(e - n * p.Lin);
    float acc = 0.0f;
    const int q = l + p.pad;
    for (int k = q % p.stride; k < p.K && k <= q; k += p.stride) {
        const int t = (q - k) / p.stride;
        if (t >= p.Lout) continue;
        const half_t* dzr = p.dz + (n * p.Lout + t) * p.Cout;
        for (int co = 0; co < p.Cout; ++co) acc = fmaf((float)dzr[co], p.w1[co * p.K + k], acc);
    }
    p.dx[e] = (half_t)acc;
}

struct ConvLayout {
    int Lout, Kp;
    size_t w, bias, dz, dw_part, db_part, total;
    ConvLayout(int N, int Lin, int Cin, int Cout, int K, int stride, int pad) {
        Lout = out_len(Lin, K, stride, pad);
        Kp = (K * Cin + 31) / 32 * 32;
        const long M = (long)N * Lout;
        const Split g(M, Cout, K * Cin);
        const size_t wbytes = Cin == 1 ? (size_t)Cout * K * sizeof(float) : (size_t)Kp * ((Cout + 15) / 16 * 16) * sizeof(half_t);
        w = 0;                                  // the packed weights come first: bh_conv1d_packed_halves(Cin, Cout, K) halves
        bias = align_up256(w + wbytes);
        dz = align_up256(bias + (size_t)Cout * sizeof(float));
        dw_part = align_up256(dz + (size_t)M * Cout * sizeof(half_t));
        db_part = align_up256(dw_part + (size_t)g.dw_splits * Cout * K * Cin * sizeof(float));
        total = align_up256(db_part + (size_t)g.db_splits * Cout * sizeof(float));
    }
};

const char* conv_shape_error(int N, int Lin, int Cin, int Cout, int K, int stride, int pad) {
    if (N < 1 || Lin < 1) return "N and Lin must be positive";
    if (!(Cin == 1 || (Cin >= 8 && Cin % 8 == 0 && Cin <= 1024))) return "Cin must be 1 or a multiple of 8 up to 1024";
    if (Cout < 4 || Cout % 4 != 0 || Cout > 4096 || (Cin == 1 && Cout > 256)) return "Cout must be a multiple of 4 (up to 4096; up to 256 for Cin == 1)";
    if (K < 1 || K > 32) return "K must be in 1..32";
    if (stride < 1 || stride > 8) return "stride must be in 1..8";
    if (pad < 0 || pad >= K) return "pad must be in 0..K-1";
    if (Lin + 2 * pad < K) return "the input is shorter than one window";
    if (Cin > 1 && ((63l * stride + K) * Cin + 40) * 2 + 16 > 160 * 1024) return "the input span of 64 positions does not fit the LDS";
    const long Lout = out_len(Lin, K, stride, pad);
    if ((long)N * ((Lout + 63) / 64) >= (1l << 31) || (long)N * Lin >= (1l << 40)) return "too many positions for one call";
    return nullptr;
}

struct LinearLayout {
    size_t w, bias, dz, dw_part, db_part, total;
    LinearLayout(int T, int N, int K, int C) {
        const long M = (long)T * N;
        const Split g(M, C, K);
        w = 0;                                  // forward: fp16 [C][K]; backward: fp16 [K][C]
        bias = align_up256(w + (size_t)C * K * sizeof(half_t));
        dz = align_up256(bias + (size_t)C * sizeof(float));
        dw_part = align_up256(dz + (size_t)M * C * sizeof(half_t));
        db_part = align_up256(dw_part + (size_t)g.dw_splits * C * K * sizeof(float));
        total = align_up256(db_part + (size_t)g.db_splits * C * sizeof(float));
    }
};

const char* linear_shape_error(int T, int N, int K, int C) {
    if (T < 1 || N < 1) return "T and N must be positive";
    if ((long)T * N >= (1l << 31)) return "T * N must stay below 2^31 rows";
    if (K < 8 || K % 8 != 0 || K > 16384) return "K must be a multiple of 8 up to 16384";
    if (C < 8 || C % 8 != 0 || C > 16384) return "C must be a multiple of 8 up to 16384";
    return nullptr;
}

struct LinearDzArgs {
    const half_t* y;
    const half_t* dy;
    half_t* dz;             // [M][C], m = t N + n
    long T, N;
    int C, act, clamped, batch_major;
    float scale, lo, hi;
};
// dz[m] = dy[row(m)] [lo < y < hi] scale act', tanh' = 1 - (y / scale)^2 from the stored y; row(m) = n T + t for batch-major y
__global__ __launch_bounds__(256) void linear_dz_kernel(LinearDzArgs p) {
    const int cv = p.C / 8;
    const long total = p.T * p.N * cv;
    const bool need_y = p.clamped || p.act == ACT_TANH;
    const float inv = 1.0f / p.scale;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long m = e / cv;
        const int c = (int)(e - m * cv) * 8;
        const long t = m / p.N, n = m - t * p.N;
        const long at = (p.batch_major ? n * p.T + t : m) * p.C + c;
        const half8_t dy8 = *(const half8_t*)(p.dy + at);
        half8_t y8 = {0, 0, 0, 0, 0, 0, 0, 0}, o;
        if (need_y) y8 = *(const half8_t*)(p.y + at);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float yv = (float)y8[j];
            const bool in = !p.clamped || (yv > p.lo && yv < p.hi);
            float g = p.scale;
            if (p.act == ACT_TANH) { const float u = yv * inv; g *= 1.0f - u * u; }
            o[j] = in ? (half_t)((float)dy8[j] * g) : (half_t)0.0f;
        }
        *(half8_t*)(p.dz + m * p.C + c) = o;
    }
}

}  // namespace
}  // namespace bh

size_t bh_k_conv_train_workspace(int N, int Lin, int Cin, int Cout, int K, int stride, int pad) {
    return bh::conv_shape_error(N, Lin, Cin, Cout, K, stride, pad) ? 0 : bh::ConvLayout(N, Lin, Cin, Cout, K, stride, pad).total;
}

// the rounded weights and bias into the workspace, in the forward's layout
static int conv_train_weights(const float* w, const float* bias, int Cin, int Cout, int K, const bh::ConvLayout& L, char* ws, hipStream_t stream) {
    using namespace bh;
    if (Cin == 1) {
        hipLaunchKernelGGL(round_kernel, dim3(cvt_grid((long)Cout * K)), dim3(256), 0, stream, w, (float*)(ws + L.w), (long)Cout * K);
    } else {
        const long total = (long)L.Kp * ((Cout + 15) / 16 * 16);
        hipLaunchKernelGGL(conv_pack_kernel, dim3(cvt_grid(total)), dim3(256), 0, stream, w, (half_t*)(ws + L.w), Cin, Cout, K, L.Kp, total);
    }
    hipLaunchKernelGGL(round_kernel, dim3(cvt_grid(Cout)), dim3(256), 0, stream, bias, (float*)(ws + L.bias), (long)Cout);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

#define CONV_TRAIN_CHECKS(what)                                                                                                              \
    const char* shape_err = conv_shape_error(N, Lin, Cin, Cout, K, stride, pad);                                                             \
    BH_REQUIRE(!shape_err, what ": %s (N=%d Lin=%d Cin=%d Cout=%d K=%d stride=%d pad=%d)", shape_err, N, Lin, Cin, Cout, K, stride, pad);  \
    BH_REQUIRE(act_ok(act), what ": unknown activation %d", act);                                                                            \
    BH_REQUIRE(clamp_lo <= clamp_hi, what ": clamp range [%g, %g] is empty", (double)clamp_lo, (double)clamp_hi);                            \
    BH_REQUIRE(os_n >= 0 && os_t >= 0 && (Cin == 1 || (os_n % 4 == 0 && os_t % 4 == 0)), what ": output strides must be multiples of 4");   \
    const ConvLayout L(N, Lin, Cin, Cout, K, stride, pad);                                                                                   \
    BH_REQUIRE(workspace_bytes >= L.total, what ": workspace of %zu bytes, bh_conv1d_train_workspace = %zu", workspace_bytes, L.total)

int bh_k_conv_train_forward(const void* x, const float* w, const float* bias, int N, int Lin, int Cin, int Cout, int K, int stride, int pad,
                            int act, float clamp_lo, float clamp_hi, long os_n, long os_t, void* y, void* workspace, size_t workspace_bytes,
                            hipStream_t stream) {
    using namespace bh;
    CONV_TRAIN_CHECKS("conv1d_train_forward");
    BH_REQUIRE(x && w && y && workspace, "conv1d_train_forward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(y) && aligned16(workspace), "conv1d_train_forward: x, y and workspace must be 16-byte aligned");
    char* ws = (char*)workspace;
    if (int rc = conv_train_weights(w, bias, Cin, Cout, K, L, ws, stream)) return rc;
    if (Cin == 1)
        return bh_k_conv_first(x, (const float*)(ws + L.w), (const float*)(ws + L.bias), y, N, Lin, L.Lout, Cout, K, stride, pad, act, clamp_lo,
                               clamp_hi, os_n, os_t, stream);
    return bh_k_conv_igemm(x, ws + L.w, (const float*)(ws + L.bias), y, N, Lin, L.Lout, Cin, Cout, K, stride, pad, act, clamp_lo, clamp_hi, os_n,
                           os_t, stream);
}

int bh_k_conv_train_backward(const void* x, const float* w, const float* bias, const void* y, const void* dy, int N, int Lin, int Cin, int Cout,
                             int K, int stride, int pad, int act, float clamp_lo, float clamp_hi, long os_n, long os_t, void* dx, float* dw,
                             float* db, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    using namespace bh;
    CONV_TRAIN_CHECKS("conv1d_train_backward");
    BH_REQUIRE(x && w && y && dy && dw && workspace, "conv1d_train_backward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(y) && aligned16(dy) && aligned16(dx) && aligned16(workspace),
               "conv1d_train_backward: x, y, dy, dx and workspace must be 16-byte aligned");
    char* ws = (char*)workspace;
    if (int rc = conv_train_weights(w, bias, Cin, Cout, K, L, ws, stream)) return rc;
    const long M = (long)N * L.Lout;
    ConvBwdArgs a{(const half_t*)x, (const half_t*)(ws + L.w), (const float*)(ws + L.w), (const float*)(ws + L.bias), (const half_t*)y,
                  (const half_t*)dy, (half_t*)(ws + L.dz), (half_t*)dx, N, Lin, L.Lout, Cin, Cout, K, stride, pad, act, L.Kp,
                  is_clamped(clamp_lo, clamp_hi) ? 1 : 0, (L.Lout + 63) / 64, clamp_lo, clamp_hi, os_n, os_t};
    if (Cin == 1)
        hipLaunchKernelGGL(conv_first_dz_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(conv_dz_kernel, dim3((unsigned)((long)N * a.tblocks), (Cout + 63) / 64), dim3(256), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    const RowRule rule{(const half_t*)x, ROWS_CONV, 0, L.Lout, Lin, Cin, stride, pad};
    if (int rc = reduce_rows(a.dz, rule, M, Cout, K * Cin, (float*)(ws + L.dw_part), (float*)(ws + L.db_part), dw, nullptr, db, stream)) return rc;
    if (dx) {
        const long items = (long)N * Lin * (Cin == 1 ? 1 : Cin / 8);
        if (Cin == 1) hipLaunchKernelGGL(conv_first_dx_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(conv_dx_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, a);
        BH_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

size_t bh_k_linear_train_workspace(int T, int N, int K, int C) {
    return bh::linear_shape_error(T, N, K, C) ? 0 : bh::LinearLayout(T, N, K, C).total;
}

#define LINEAR_TRAIN_CHECKS(what)                                                                                                  \
    const char* shape_err = linear_shape_error(T, N, K, C);                                                                        \
    BH_REQUIRE(!shape_err, what ": %s (T=%d N=%d K=%d C=%d)", shape_err, T, N, K, C);                                             \
    BH_REQUIRE(act == ACT_NONE || act == ACT_TANH, what ": activation %d is not supported (none or tanh)", act);                   \
    BH_REQUIRE(scale != 0.0f && std::isfinite(scale), what ": scale must be finite and not 0");                                    \
    BH_REQUIRE(clamp_lo <= clamp_hi, what ": clamp range [%g, %g] is empty", (double)clamp_lo, (double)clamp_hi);                  \
    BH_REQUIRE(batch_major == 0 || batch_major == 1, what ": batch_major must be 0 or 1 (got %d)", batch_major);                   \
    const LinearLayout L(T, N, K, C);                                                                                              \
    BH_REQUIRE(workspace_bytes >= L.total, what ": workspace of %zu bytes, bh_linear_train_workspace = %zu", workspace_bytes, L.total)

int bh_k_linear_train_forward(const void* x, const float* w, const float* bias, int T, int N, int K, int C, int act, float scale,
                              float clamp_lo, float clamp_hi, int batch_major, void* y, void* workspace, size_t workspace_bytes,
                              hipStream_t stream) {
    using namespace bh;
    LINEAR_TRAIN_CHECKS("linear_train_forward");
    BH_REQUIRE(x && w && y && workspace, "linear_train_forward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(y) && aligned16(workspace), "linear_train_forward: x, y and workspace must be 16-byte aligned");
    char* ws = (char*)workspace;
    half_t* w16 = (half_t*)(ws + L.w);
    float* b16 = bias ? (float*)(ws + L.bias) : nullptr;
    if (int rc = round_weights(w, w16, C, K, WEIGHTS_ROWS, stream)) return rc;
    if (bias) hipLaunchKernelGGL(round_kernel, dim3(cvt_grid(C)), dim3(256), 0, stream, bias, b16, (long)C);
    BH_CHECK_HIP(hipGetLastError());
    return linear_rows((const half_t*)x, w16, b16, (half_t*)y, T, N, K, C, act, scale, clamp_lo, clamp_hi, batch_major != 0, false, stream);
}

int bh_k_linear_train_backward(const void* x, const float* w, const void* y, const void* dy, int T, int N, int K, int C, int act, float scale,
                               float clamp_lo, float clamp_hi, int batch_major, void* dx, float* dw, float* db, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
    using namespace bh;
    LINEAR_TRAIN_CHECKS("linear_train_backward");
    BH_REQUIRE(x && w && y && dy && dw && workspace, "linear_train_backward: null pointer");
    BH_REQUIRE(aligned16(x) && aligned16(y) && aligned16(dy) && aligned16(dx) && aligned16(workspace),
               "linear_train_backward: x, y, dy, dx and workspace must be 16-byte aligned");
    char* ws = (char*)workspace;
    half_t* wT = (half_t*)(ws + L.w);
    half_t* dz = (half_t*)(ws + L.dz);
    const long rows = (long)T * N;
    LinearDzArgs a{(const half_t*)y, (const half_t*)dy, dz, T, N, C, act, is_clamped(clamp_lo, clamp_hi) ? 1 : 0, batch_major, scale, clamp_lo,
                   clamp_hi};
    const long items = rows * (C / 8);
    hipLaunchKernelGGL(linear_dz_kernel, dim3((unsigned)((items + 255) / 256 < 65536 ? (items + 255) / 256 : 65536)), dim3(256), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    if (dx) {      // dx = dz W over all rows, fp16
        if (int rc = round_weights(w, wT, C, K, WEIGHTS_TRANSPOSED, stream)) return rc;
        if (int rc = linear_rows(dz, wT, nullptr, (half_t*)dx, T, N, C, K, ACT_NONE, 1.0f, -INFINITY, INFINITY, false, false, stream)) return rc;
    }
    const RowRule rule{(const half_t*)x, ROWS_PLAIN, K};
    return reduce_rows(dz, rule, rows, C, K, (float*)(ws + L.dw_part), (float*)(ws + L.db_part), dw, nullptr, db, stream);
}
