// 1-D convolution front-end for gfx950 (replaces cuDNN behind bonito.nn.Convolution,
// the reference's bonito/nn.py:222-241, with BatchNorm already folded as nn.py:447-454 does).
//
// Activations between convolutions are kept CHANNEL-MINOR ([N][L][C] fp16). With that layout the
// im2col row of output position t -- all (k, c) taps -- is ONE contiguous run of K*Cin halves
// starting at input position t*stride - pad, so the convolution is an implicit GEMM whose B
// fragments are plain 16-byte LDS reads with no gather:
//     out[t][f] = sum_{kk < K*Cin} Wp[f][kk] * in_flat[(t*stride - pad)*Cin + kk]
// Wp is the conv weight re-packed [Cout][k*Cin + c] and zero-padded to a multiple of 32.
//
//  * bh_k_conv_first : Cin == 1 (raw signal, [N][L] fp16) on the VALU, writes channel-minor.
//  * bh_k_conv_igemm : Cin % 8 == 0 on MFMA 16x16x32 f16; W is the A operand so a lane owns 4
//    consecutive output features of one position (8-byte packed stores, lane-local epilogue).
//    The output may be written NTC ([N][T][C]) or TNC ([T][N][C], what the LSTM stack consumes;
//    this folds nn.Permute([2,0,1]), nn.py:331-338, into the store). Two kernels behind it:
//    conv_igemm_kernel (any shape) and conv_ws_kernel (weight-stationary, the layer in front of the LSTM stack).
//  * bh_k_conv_front3 : conv1 -> conv2 -> conv3 of an LSTM model's front end in one kernel (conv_front3_kernel, or
//    conv_front3_pipe_kernel, which runs conv1 / conv2 of the next block beside conv3).
//  * bh_k_conv_front3_ok / _shape_ok / _option_ok : may the engine (the launcher, the options) take bh_k_conv_front3?
//  * bh_k_conv_last_kernel / bh_k_conv_note_kernel : test hook, the kernel and instance of the last convolution launch.
//
// Every kernel body is a sequence of stages, each written once as a __device__ function (stage_span, act_inplace, conv1_rows, conv2_tile,
// ws_block ...). Front3Lds and PipeLds lay out the LDS of the fused kernels for kernel and launcher alike. The instances are rows of
// IGEMM_INSTANCES and WS_INSTANCES; every launch goes through conv_launch.
#include "common.h"
#include "kernels.h"
#include "options.h"
#include <cstring>

namespace bh {

// ---------------------------------------------------------------------------------------------
struct ConvFirstArgs {
    const half_t* sig;  // [N][Lin]
    const float* w;     // [Cout][K]
    const float* bias;  // [Cout]
    half_t* out;
    int N, Lin, Lout, Cout, K, stride, pad, act;
    float clamp_lo, clamp_hi;
    long os_n, os_t;
    int vec8;
};

__global__ __launch_bounds__(256) void conv_first_kernel(ConvFirstArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* wl = (float*)smem;           // [Cout][K]
    float* bl = wl + p.Cout * p.K;      // [Cout]
    float* sl = bl + p.Cout;            // signal span of this workgroup, zero padded
    const int n = blockIdx.y;
    const int tb = blockIdx.x * 256;
    const int span = 255 * p.stride + p.K;
    const half_t* s = p.sig + (long)n * p.Lin;
    for (int i = threadIdx.x; i < p.Cout * p.K; i += 256) wl[i] = p.w[i];
    for (int i = threadIdx.x; i < p.Cout; i += 256) bl[i] = p.bias ? p.bias[i] : 0.0f;
    for (int i = threadIdx.x; i < span; i += 256) {
        int pos = tb * p.stride - p.pad + i;
        sl[i] = (pos >= 0 && pos < p.Lin) ? (float)s[pos] : 0.0f;
    }
    __syncthreads();
    const int t = tb + threadIdx.x;
    if (t >= p.Lout) return;
    const float* x = sl + threadIdx.x * p.stride;
    half_t* dst = p.out + (long)n * p.os_n + (long)t * p.os_t;
    auto channel = [&](int c) {
        const float* wr = wl + c * p.K;
        float a = bl[c];
        for (int k = 0; k < p.K; ++k) a = fmaf(wr[k], x[k], a);
        a = apply_act_rt(a, p.act);
        return (half_t)fminf(fmaxf(a, p.clamp_lo), p.clamp_hi);
    };
    int c0 = 0;
    if (p.vec8) {   // Cout and both output strides are multiples of 8: 16-byte packed stores
        if (p.K == 5 && p.act == ACT_SWISH) {       // every bonito model: taps unrolled, the activation switch outside the channel loop
            const float x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4];
            for (; c0 + 8 <= p.Cout; c0 += 8) {
                half8_t o;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float* wr = wl + (c0 + j) * 5;
                    float a = bl[c0 + j];
                    a = fmaf(wr[0], x0, a);
                    a = fmaf(wr[1], x1, a);
                    a = fmaf(wr[2], x2, a);
                    a = fmaf(wr[3], x3, a);
                    a = fmaf(wr[4], x4, a);
                    o[j] = (half_t)fminf(fmaxf(swishf_(a), p.clamp_lo), p.clamp_hi);
                }
                *(half8_t*)(dst + c0) = o;
            }
        }
        for (; c0 + 8 <= p.Cout; c0 += 8) {
            half8_t o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = channel(c0 + j);
            *(half8_t*)(dst + c0) = o;
        }
    }
    for (; c0 < p.Cout; ++c0) dst[c0] = channel(c0);
}

// ---------------------------------------------------------------------------------------------
struct ConvArgs {
    const half_t* in;   // [N][Lin][Cin]
    const half_t* wpk;  // [Cout16][Kp]
    const float* bias;  // [Cout]
    half_t* out;
    int N, Lin, Lout, Cin, Cout, K, stride, pad, act;
    int Kp;             // padded K*Cin (multiple of 32)
    float clamp_lo, clamp_hi;
    long os_n, os_t;
};

// ---- stages shared by the kernels below -------------------------------------------------------------------------------------------
// The clamp as ONE instruction, v_med3_f32, where fminf(fmaxf(x, lo), hi) is three (the compiler puts a canonicalising v_max in front of
// the pair): the same value for lo <= hi - x itself inside, the bound outside, and lo for a NaN (of three operands with a NaN the
// instruction returns their minimum, which skips the NaN) - so the same bytes (2048 x 10000: 1.31 -> 1.22 ms over the three layers).
// conv_front3_pipe_kernel clamps with it (MED3), every other kernel with the pair.
static __device__ __forceinline__ float clamp_med3(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }
template <bool MED3>
static __device__ __forceinline__ float clampf(float x, float lo, float hi) {
    if constexpr (MED3) return clamp_med3(x, lo, hi);
    else return fminf(fmaxf(x, lo), hi);
}

// The activation of a few outputs with the switch of apply_act_rt once per group, not once per output: swish (every bonito model)
// straight, anything else through the switch.
template <int N>
static __device__ __forceinline__ void act_inplace(float (&v)[N], int act) {
    if (act == ACT_SWISH) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = swishf_(v[i]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = apply_act_rt(v[i], act);
    }
}

// The contiguous input span of PB output positions: (PB - 1) * stride + K positions of Cin halves, and the tail read by the zero-padded
// K columns. The kernels stage and index by it, the launchers size the LDS by it.
struct ConvSpan {
    int pos, halves;
    __host__ __device__ ConvSpan(int PB, int stride, int K, int Cin) : pos((PB - 1) * stride + K), halves(pos * Cin + 32 + 8) {}
    __host__ __device__ size_t bytes() const { return (size_t)halves * 2 + 16; }
};

// stage the span of the block at output position t0 of chunk n (zero outside [0, Lin)), NT threads
template <int NT>
static __device__ __forceinline__ void stage_span(half_t* xin, const ConvArgs& p, const ConvSpan& sp, int n, int t0, int tid) {
    const int p_start = t0 * p.stride - p.pad;
    const half_t* src = p.in + (long)n * p.Lin * p.Cin;
    for (int e = tid * 8; e < sp.halves; e += NT * 8) {
        int pos = p_start + e / p.Cin;
        uint4_t v = {0, 0, 0, 0};
        if (pos >= 0 && pos < p.Lin && e < sp.pos * p.Cin)
            v = *(const uint4_t*)(src + (long)pos * p.Cin + (e % p.Cin));
        *(uint4_t*)(xin + e) = v;
    }
}

// FS (round 4, layers with a multiple of 64 output channels): the four waves split the FEATURE tiles and each covers all 4 * NTT
// position tiles of the workgroup, instead of splitting the positions and each walking all feature tiles: a weight fragment is then
// fetched once per workgroup (not once per wave) and feeds 4 * NTT MFMAs instead of NTT. Same accumulation order per output.
template <int NTT, bool FS = false>  // position tiles (of 16) per wave and feature tile
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* xin = (half_t*)smem;
    constexpr int PW = NTT * 16;
    constexpr int PB = 4 * PW;  // positions per workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kg = lane >> 4;
    const int n = blockIdx.y;
    const int t0 = blockIdx.x * PB;

    stage_span<256>(xin, p, ConvSpan(PB, p.stride, p.K, p.Cin), n, t0, tid);
    __syncthreads();

    const int nks = p.Kp >> 5;
    const int nft = (p.Cout + 15) >> 4;
    constexpr int NT = FS ? 4 * NTT : NTT;           // position tiles this wave covers
    const int pbase = FS ? 0 : wave * PW;
    int boff[NT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
        boff[tt] = (pbase + tt * 16 + r) * p.stride * p.Cin + kg * 8;

    for (int ft = FS ? wave : 0; ft < nft; ft += FS ? 4 : 1) {
        float4_t acc[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) acc[tt] = float4_t{0.f, 0.f, 0.f, 0.f};
        const half_t* wrow = p.wpk + (long)(ft * 16 + r) * p.Kp + kg * 8;
        // four k-steps per trip: their weight fragments (global, L2-resident) are requested together, so a trip waits for one round
        // trip instead of four (one k-step per trip left 1-2 MFMAs per exposed load at 16 / 32 positions per wave)
        int ks = 0;
        for (; FS && ks + 4 <= nks; ks += 4) {       // (FS instances only: the 16-channel layers of the LSTM models have 3 k-steps and measured 5-10 % slower with this loop in front of theirs)
            half8_t a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = *(const half8_t*)(wrow + (ks + u) * 32);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) {
                    half8_t b = *(const half8_t*)(xin + boff[tt] + (ks + u) * 32);
                    acc[tt] = mfma16(a[u], b, acc[tt]);
                }
        }
        for (; ks < nks; ++ks) {
            half8_t a = *(const half8_t*)(wrow + ks * 32);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
                half8_t b = *(const half8_t*)(xin + boff[tt] + ks * 32);
                acc[tt] = mfma16(a, b, acc[tt]);
            }
        }
        const int f = ft * 16 + kg * 4;
        if (f < p.Cout) {
            float bv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) bv[g] = (p.bias && f + g < p.Cout) ? p.bias[f + g] : 0.0f;
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
                int t = t0 + pbase + tt * 16 + r;
                if (t >= p.Lout) continue;
                float xv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) xv[g] = acc[tt][g] + bv[g];
                // (act_inplace written out: through the function the epilogue of the unrolled tiles comes out with three times the
                // branches, and the 5-tap 384-channel layer measured 4 % slower)
                if (p.act == ACT_SWISH) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) xv[g] = swishf_(xv[g]);
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g) xv[g] = apply_act_rt(xv[g], p.act);
                }
                half4_t o;
#pragma unroll
                for (int g = 0; g < 4; ++g) o[g] = (half_t)fminf(fmaxf(xv[g], p.clamp_lo), p.clamp_hi);
                half_t* dst = p.out + (long)n * p.os_n + (long)t * p.os_t + f;
                if (f + 4 <= p.Cout) *(half4_t*)dst = o;
                else
                    for (int g = 0; g < 4; ++g)
                        if (f + g < p.Cout) dst[g] = o[g];
            }
        }
    }
}

// Weight-stationary variant for the layer that feeds the recurrent stack (conv3: 16 -> 384 channels in hac-sized models,
// 16 -> 96 in fast-sized ones; 19 taps): the WAVES waves of a workgroup split the feature tiles (FPW each) and keep their weight fragments in registers for the whole block of 256
// output positions; every wave walks the 16 position tiles, reading each tile's NKS input fragments from LDS once and
// using them for FPW MFMAs each. There is no global load inside the loop, so nothing ever waits on `vmcnt` and the output
// stores stream out behind the arithmetic (in conv_igemm_kernel the wait for the next tile's weights also drains the
// previous tile's stores: loads and stores share one in-order counter on gfx950). Same accumulation order as
// conv_igemm_kernel (k-steps ascending into one accumulator), so the two kernels give identical bytes.

// a wave's weight fragments: FPW feature tiles x NKS k-steps
template <int FPW, int NKS>
static __device__ __forceinline__ void ws_load_fragments(half8_t (&afr)[FPW][NKS], const ConvArgs& p, int wave, int r, int kg) {
#pragma unroll
    for (int f = 0; f < FPW; ++f) {
        const half_t* wrow = p.wpk + (long)((wave * FPW + f) * 16 + r) * p.Kp + kg * 8;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) afr[f][ks] = *(const half8_t*)(wrow + ks * 32);
    }
}

// Where ws_block takes a wave's biases from. In registers, loaded once per kernel:
template <int FPW>
struct WsBiasRegs {
    float4_t bv[FPW];
    __device__ __forceinline__ WsBiasRegs(const float* bias, int wave, int kg) {
#pragma unroll
        for (int f = 0; f < FPW; ++f) {
            bv[f] = float4_t{0.f, 0.f, 0.f, 0.f};
            if (bias) bv[f] = *(const float4_t*)(bias + (wave * FPW + f) * 16 + kg * 4);
        }
    }
    __device__ __forceinline__ void add(float4_t (&acc)[FPW]) const {
#pragma unroll
        for (int f = 0; f < FPW; ++f)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[f][g] += bv[f][g];
    }
};
// ... or from LDS tile by tile (conv_front3_pipe_kernel; the offset is opaque, so that the reads stay in the loop over the tiles): the
// weight fragments leave no twelve registers to hold them in, and spilled fragments are reloaded in that loop
template <int FPW>
struct WsBiasLds {
    const float* b3l;   // [16 * FPW * waves], zeros without a bias
    int wave, kg;
    __device__ __forceinline__ void add(float4_t (&acc)[FPW]) const {
        int bo = (wave * FPW * 16 + kg * 4) * 4;
        asm volatile("" : "+v"(bo));
#pragma unroll
        for (int f = 0; f < FPW; ++f) {
            const float4_t bv = *(const float4_t*)((const char*)b3l + bo + f * 64);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[f][g] += bv[g];
        }
    }
};

template <int ACT, int FPW>
static __device__ __forceinline__ void ws_act(float4_t (&acc)[FPW]) {
#pragma unroll
    for (int f = 0; f < FPW; ++f)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[f][g] = apply_act<ACT>(acc[f][g]);
}

// One block of 256 output positions from the span buffer xin (rows of RS halves per output position): every wave walks the 16 position
// tiles with its fragments afr, k-steps ascending into one accumulator, the bias behind them, activation, clamp, 8-byte stores.
// UNROLL: copies of the tile loop's body, 16 (all tiles) or 1. Stated, because the compiler's own choice follows accidents of the
// surrounding code: written out in the kernels, the three-tile-per-wave instances came out with all 16 tiles unrolled and every other
// one rolled, and as a function all came out rolled. The callers ask for what they have always been built as (WS_UNROLL below).
template <int FPW, int NKS, bool MED3, int UNROLL, class Bias>
static __device__ __forceinline__ void ws_block(const half8_t (&afr)[FPW][NKS], const Bias& bias, const half_t* xin, int RS, const ConvArgs& p,
                                                int n, int t0, int wave, int r, int kg) {
#pragma unroll UNROLL
    for (int pt = 0; pt < 256 / 16; ++pt) {
        const int t = t0 + pt * 16 + r;
        if (t0 + pt * 16 >= p.Lout) break;
        const half_t* xrow = xin + (pt * 16 + r) * RS + kg * 8;
        half8_t b[NKS];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) b[ks] = *(const half8_t*)(xrow + ks * 32);
        float4_t acc[FPW];
#pragma unroll
        for (int f = 0; f < FPW; ++f) acc[f] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int f = 0; f < FPW; ++f) acc[f] = mfma16(afr[f][ks], b[ks], acc[f]);
        bias.add(acc);
        switch (p.act) {                              // (once per tile, not once per output)
            case ACT_SWISH: ws_act<ACT_SWISH>(acc); break;
            case ACT_TANH: ws_act<ACT_TANH>(acc); break;
            case ACT_RELU: ws_act<ACT_RELU>(acc); break;
            default: break;
        }
        if (t < p.Lout) {
            half_t* drow = p.out + (long)n * p.os_n + (long)t * p.os_t + kg * 4;
#pragma unroll
            for (int f = 0; f < FPW; ++f) {
                half4_t o;
#pragma unroll
                for (int g = 0; g < 4; ++g) o[g] = (half_t)clampf<MED3>(acc[f][g], p.clamp_lo, p.clamp_hi);
#ifdef BH_CONV_EXPT_NOSTORE       // timing experiment (wrong results): the kernels without conv3's output stores
                if (o[0] == (half_t)12345.0f)
#endif
                *(half4_t*)(drow + (wave * FPW + f) * 16) = o;
            }
        }
    }
}

// the tile loop of conv_ws_kernel and conv_front3_kernel: unrolled with three feature tiles per wave (384 channels); with one (96 channels)
// rolled - unrolled, conv_ws_kernel<1, 10, 6> takes 66 registers and loses its eighth wave per SIMD
template <int FPW>
constexpr int WS_UNROLL = FPW > 1 ? 16 : 1;

template <int FPW, int NKS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void conv_ws_kernel(ConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* xin = (half_t*)smem;
    constexpr int PB = 256;                    // positions per workgroup = 16 tiles of 16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kg = lane >> 4;
    const int n = blockIdx.y;
    const int t0 = blockIdx.x * PB;

    // this wave's weight fragments and biases (requested first, they land during the staging)
    half8_t afr[FPW][NKS];
    ws_load_fragments(afr, p, wave, r, kg);
    const WsBiasRegs<FPW> bias(p.bias, wave, kg);
    stage_span<64 * WAVES>(xin, p, ConvSpan(PB, p.stride, p.K, p.Cin), n, t0, tid);
    __syncthreads();
    ws_block<FPW, NKS, false, WS_UNROLL<FPW>>(afr, bias, xin, p.stride * p.Cin, p, n, t0, wave, r, kg);
}

// ---------------------------------------------------------------------------------------------
// Fused front-end (round 4): conv1 (1 -> 16 channels, VALU) -> conv2 (16 -> 16, MFMA) -> conv3 (the weight-stationary
// kernel above) in ONE kernel. The 16-channel intermediates never leave the CU: a workgroup of conv3 needs conv2's outputs for its span
// of (PB - 1) * stride + K positions, which it now COMPUTES into the LDS buffer conv_ws_kernel used to fill from global memory - in
// chunks of 256 positions: conv1 of the chunk (+ K2 - 1 halo rows) from the staged signal into a small LDS buffer, a barrier, conv2 of
// the chunk by MFMA from there into the span buffer, a barrier. The halo is recomputed (1.6 % of conv1 / conv2), 0.33 GB of writes and
// 0.33 GB of reads per hac batch are gone, and two launches. Every output is computed by the operations of the three separate kernels
// in their order (conv1: bias + fmaf over the taps; conv2: the same three k-steps into one accumulator, bias added behind them;
// positions outside a layer's output are the ZEROS of the next layer's padding, not evaluations on a padded input): identical bytes
// (tests/test_gpu_ops.py::test_fused_conv_front_end_equals_three_kernels, "conv_fuse" 0 restores the three kernels).
struct ConvFront3Args {
    const half_t* sig;     // [N][L0]
    const float* w1;       // [16][K1]
    const float* b1;       // [16]
    const half_t* w2pk;    // [16][Kp2], Kp2 = K2 * 16 rounded up to 32 (<= 96), as bh_conv1d_pack lays it out
    const float* b2;       // [16]
    int L0, L1, L2;        // lengths: signal, conv1 output, conv2 output
    int K1, pad1, act1;
    int K2, pad2, act2;
    float lo1, hi1, lo2, hi2;
    ConvArgs c3;           // conv3 exactly as conv_ws_kernel takes it (c3.in unused, c3.Lin = L2)
};

// LDS of conv_front3_kernel, for the kernel (pointers) and the launcher (bytes): byte offsets of the regions behind the span buffer
struct Front3Lds {
    int span_pos, span_halves;     // conv2 positions conv3 reads; halves of the span buffer with its tail
    int a1_rows;                   // conv1 outputs of one chunk [256 + K2 - 1 (+ 6 rows read by the zero-padded k columns)][16]
    int a1, sl, wl, bl, bytes;     // xin [span_pos][16] (+ tail) at 0 | a1 | signal span, zero padded | conv1 weights [16][K1] | bias [16]
    __host__ __device__ Front3Lds(int K1, int K2, int K3, int s3) {
        const ConvSpan sp(256, s3, K3, 16);
        span_pos = sp.pos, span_halves = sp.halves;
        a1_rows = 256 + K2 - 1 + 6;
        a1 = ((span_halves + 7) & ~7) * 2;
        sl = a1 + a1_rows * 16 * 2;
        wl = sl + (span_pos + K2 - 1 + K1 - 1 + 8) * 4;
        bl = wl + 16 * K1 * 4;
        bytes = bl + 16 * 4;
    }
};

// conv1's work item: eight channels (c0 = 0 or 8) of one position into a half8, from x = the position's first tap in the signal strip;
// outside conv1's output it is conv2's zero padding. K1 == 5 (every bonito model): the thread's 40 weights and 8 biases live in registers
// (conv1_load5) and the taps are unrolled - with the generic loop (two LDS reads in front of every dependent fmaf, eight waves per CU
// to hide them) this phase took longer than conv3 itself
static __device__ __forceinline__ void conv1_load5(float (&w1r)[8][5], float (&w1b)[8], const float* wl, const float* bl, int c0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        w1b[c] = bl[c0 + c];
#pragma unroll
        for (int k = 0; k < 5; ++k) w1r[c][k] = wl[(c0 + c) * 5 + k];
    }
}
template <bool MED3>
static __device__ __forceinline__ half8_t conv1_item5(const float* x, const float (&w1r)[8][5], const float (&w1b)[8], int act, bool inside,
                                                      float lo, float hi) {
    const float x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4];
    float av[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float a = w1b[c];
        a = fmaf(w1r[c][0], x0, a);
        a = fmaf(w1r[c][1], x1, a);
        a = fmaf(w1r[c][2], x2, a);
        a = fmaf(w1r[c][3], x3, a);
        a = fmaf(w1r[c][4], x4, a);
        av[c] = a;
    }
    act_inplace(av, act);
    half8_t o;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = inside ? (half_t)clampf<MED3>(av[c], lo, hi) : (half_t)0.0f;
    return o;
}
static __device__ __forceinline__ half8_t conv1_item(const float* x, const float* wl, const float* bl, int c0, int K1, int act, bool inside,
                                                     float lo, float hi) {                  // generic tap count
    half8_t o;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float* wr = wl + (c0 + c) * K1;
        float a = bl[c0 + c];
        for (int k = 0; k < K1; ++k) a = fmaf(wr[k], x[k], a);
        a = apply_act_rt(a, act);
        const half_t hv = (half_t)fminf(fmaxf(a, lo), hi);
        o[c] = inside ? hv : (half_t)0.0f;
    }
    return o;
}
// conv1 into the row buffer a1: items w = w_lo, w_lo + STEP, ... < w_hi, item w = channels c0 (the caller's w & 1, fixed per thread: STEP
// is even) of a1 row i = w >> 1 = conv1 position u0 + i, whose first tap is x[i]
template <bool MED3, int STEP>
static __device__ __forceinline__ void conv1_rows(half_t* a1, const float* x, int u0, int w_lo, int w_hi, int c0, const float (&w1r)[8][5],
                                                  const float (&w1b)[8], const float* wl, const float* bl, const ConvFront3Args& q) {
    if (q.K1 == 5) {
        for (int w = w_lo; w < w_hi; w += STEP) {
            const int i = w >> 1, u = u0 + i;
            *(half8_t*)(a1 + i * 16 + c0) = conv1_item5<MED3>(x + i, w1r, w1b, q.act1, u >= 0 && u < q.L1, q.lo1, q.hi1);
        }
    } else {
        for (int w = w_lo; w < w_hi; w += STEP) {
            const int i = w >> 1, u = u0 + i;
            *(half8_t*)(a1 + i * 16 + c0) = conv1_item(x + i, wl, bl, c0, q.K1, q.act1, u >= 0 && u < q.L1, q.lo1, q.hi1);
        }
    }
}

// conv2's three weight fragments and bias
// (the packer pads a row to Kp2 = K2 * 16 rounded up to 32 halves: 96 for the models' K2 = 5, 32 / 64 for K2 <= 4, whose missing
// k-steps are zero fragments here - they add exact zeros to the accumulator, the bytes stay those of conv_igemm_kernel's one or two steps)
static __device__ __forceinline__ void conv2_load(half8_t (&a2)[3], float (&b2v)[4], const half_t* w2pk, const float* b2, int K2, int r, int kg) {
    const int kp2 = ((K2 * 16 + 31) >> 5) << 5;
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
        a2[ks] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        if (ks * 32 < kp2) a2[ks] = *(const half8_t*)(w2pk + (long)r * kp2 + kg * 8 + ks * 32);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) b2v[g] = b2 ? b2[kg * 4 + g] : 0.0f;
}
// One 16-row tile of conv2 from xrow (this lane's row of conv1 outputs: K = K2 * 16 halves of a row run, padded to 96 with zero weights)
// into span row j = conv2 position p3_start + j of xin: the lane's four channels; outside conv2's output it is conv3's zero padding
template <bool MED3>
static __device__ __forceinline__ void conv2_tile(const half8_t (&a2)[3], const float (&b2v)[4], const half_t* xrow, half_t* xin, int j,
                                                  int p3_start, int span_pos, int kg, const ConvFront3Args& q) {
    const int v = p3_start + j;
    const bool inside = v >= 0 && v < q.L2;
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) acc = mfma16(a2[ks], *(const half8_t*)(xrow + ks * 32), acc);
    float xv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) xv[g] = acc[g] + b2v[g];
    act_inplace(xv, q.act2);
    half4_t o;
#pragma unroll
    for (int g = 0; g < 4; ++g) o[g] = inside ? (half_t)clampf<MED3>(xv[g], q.lo2, q.hi2) : (half_t)0.0f;
    if (j < span_pos) *(half4_t*)(xin + j * 16 + kg * 4) = o;
}

template <int FPW, int NKS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void conv_front3_kernel(ConvFront3Args q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ConvArgs& p = q.c3;
    constexpr int PB = 256, CH = 256, C16 = 16, NT = 64 * WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kg = lane >> 4;
    const int n = blockIdx.y;
    const int t0 = blockIdx.x * PB;
    const Front3Lds L(q.K1, q.K2, p.K, p.stride);
    const int span_pos = L.span_pos, span_halves = L.span_halves, a1_rows = L.a1_rows;
    half_t* xin = (half_t*)smem;
    half_t* a1 = (half_t*)(smem + L.a1);
    float* sl = (float*)(smem + L.sl);
    float* wl = (float*)(smem + L.wl);
    float* bl = (float*)(smem + L.bl);

    // (conv3's 120 registers of fragments are fetched behind the front phase: held across it they pushed the kernel to the register limit)
    half8_t a2[3];
    float b2v[4];
    conv2_load(a2, b2v, q.w2pk, q.b2, q.K2, r, kg);

    // ---- signal span and conv1's weights -> LDS ----------------------------------------------------------------------------------
    const int p3_start = t0 * p.stride - p.pad;                       // conv2 position of span row 0
    const int s_start = p3_start - q.pad2 - q.pad1;                   // signal position of sl[0]
    const int s_len = span_pos + q.K2 - 1 + q.K1 - 1;
    const half_t* sg = q.sig + (long)n * q.L0;
    for (int i = tid; i < s_len; i += NT) {
        const int pos = s_start + i;
        sl[i] = (pos >= 0 && pos < q.L0) ? (float)sg[pos] : 0.0f;
    }
    for (int i = tid; i < C16 * q.K1; i += NT) wl[i] = q.w1[i];
    if (tid < C16) bl[tid] = q.b1 ? q.b1[tid] : 0.0f;
    for (int e = span_pos * C16 + tid; e < span_halves; e += NT) xin[e] = (half_t)0.0f;     // tail read by conv3's zero-padded k columns
    for (int e = (CH + q.K2 - 1) * C16 + tid; e < a1_rows * C16; e += NT) a1[e] = (half_t)0.0f;   // ... and by conv2's
    __syncthreads();
    const int c0t = (tid & 1) * 8;                                    // fixed per thread: NT is even
    float w1r[8][5], w1b[8];
    if (q.K1 == 5) conv1_load5(w1r, w1b, wl, bl, c0t);

    // ---- conv1 -> conv2 -> span buffer, 256 positions of conv2 at a time ---------------------------------------------------------
    for (int q0 = 0; q0 < span_pos; q0 += CH) {
        // conv1 rows of this chunk: a1 row i = conv1 position u = p3_start + q0 - pad2 + i, i < CH + K2 - 1; its first tap is signal
        // position u - pad1 = s_start + q0 + i
        const int rows1 = min(CH, span_pos - q0) + q.K2 - 1;
        conv1_rows<false, NT>(a1, sl + q0, p3_start + q0 - q.pad2, tid, 2 * rows1, c0t, w1r, w1b, wl, bl, q);
        __syncthreads();
        // conv2 of the chunk: position tiles wave, wave + WAVES, ...
        const int tiles = (min(CH, span_pos - q0) + 15) >> 4;
        for (int pt = wave; pt < tiles; pt += WAVES)
            conv2_tile<false>(a2, b2v, a1 + (pt * 16 + r) * C16 + kg * 8, xin, q0 + pt * 16 + r, p3_start, span_pos, kg, q);
        __syncthreads();
    }

    // ---- conv3: conv_ws_kernel's block on the span buffer ---------------------------------------------------------------------------
    half8_t afr[FPW][NKS];
    ws_load_fragments(afr, p, wave, r, kg);
    const WsBiasRegs<FPW> bias(p.bias, wave, kg);
    ws_block<FPW, NKS, false, WS_UNROLL<FPW>>(afr, bias, xin, p.stride * C16, p, n, t0, wave, r, kg);
}

// ---------------------------------------------------------------------------------------------
// The fused front end as a pipeline ("conv_front_pipe", 384-channel stacks): conv1 / conv2 of block k + 1 run BESIDE conv3 of block k.
// conv_front3_kernel's one workgroup per CU (166 registers: 3 waves per SIMD, and 8 waves are one workgroup) runs its phases one after
// another - while conv1 issues on the VALU the matrix pipe idles, while conv3's MFMAs run the wave's own VALU waits. Here a workgroup
// is 12 waves, exactly what a CU holds at 168 registers:
//  * waves 0-7, the CONSUMERS, are conv_front3_kernel's conv3 loop (weight fragments in registers, fetched once per workgroup, the same
//    MFMA order and epilogue) on one of TWO span buffers;
//  * waves 8-11, the PRODUCERS (one per SIMD), fill the other span buffer for the next block. Each is self-contained: it takes a
//    contiguous quarter of the span's 16-row tiles and walks it in slices of 64 conv2 rows - the slice's signal into a private LDS
//    strip, conv1 of the slice into a private [64 + K2 - 1] row buffer (the K2 - 1 halo rows are computed once per quarter and carried
//    from slice to slice by a copy, so a slice is two WHOLE passes of 64 conv1 items - no 520-of-512 straggler), then conv2 of its
//    four tiles into the span buffer. Producers never wait on each other; within a wave LDS operations complete in order.
//  * ONE workgroup barrier per block. A workgroup walks a contiguous run of (chunk, block) pairs (grid: at most one workgroup per CU,
//    runs split evenly), so the pipeline fills and drains once per run. Workgroups never wait on each other.
// The two roles are two loops, not two branches in one loop: registers are allocated per kernel, and conv3's 132 registers of weight
// fragments and biases, live through a shared loop body, would leave conv1 36. BOTH LOOPS RUN it = 0 .. nrun WITH EXACTLY ONE BARRIER
// PER TRIP, nrun is computed in front of the split, and nothing inside a trip leaves it early: every wave executes 1 + (nrun + 1)
// barriers. At trip `it` the producers write buffer it & 1 and the consumers read buffer (it - 1) & 1.
// Arithmetic: that of conv_front3_kernel operation for operation (identical bytes: tests/test_gpu_conv_front_pipeline.py). A last
// block with few positions produces only the span rows its position tiles read (through the zero-weight twentieth row); what the
// other rows of the buffer hold reaches only MFMA columns of positions that are not stored.

static __device__ __forceinline__ void wave_lds_sync() {       // orders this wave's LDS traffic across its lanes (the hardware keeps a wave's LDS operations in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int PIPE_CW = 8, PIPE_PW = 4, PIPE_SL = 64;             // consumer waves, producer waves, conv2 rows per producer slice
constexpr int PIPE_A1R = PIPE_SL + 5 + 7;                         // rows of a producer's conv1 buffer: slice + halo (K2 <= 6) + rows under conv2's zero-padded k columns
constexpr int PIPE_NSV = (PIPE_SL + 12 + 63) / 64;                   // samples of a strip per lane
constexpr int PIPE_SG = PIPE_SL + 5 + 7 + 4;                      // floats of a producer's signal strip: slice + K2 - 1 + K1 - 1 (K1 <= 8)

// LDS of conv_front3_pipe_kernel, for the kernel (pointers) and the launcher (bytes); c3 = conv3's channels = 16 * FPW * PIPE_CW
// (at most 128 KiB: stride 7, 20 taps)
struct PipeLds {
    int span_pos, span_halves, xin_halves;
    int a1, sl, wl, bl, b3, bytes;   // two span buffers [span_pos][16] (+ tail) at 0 | the producers' conv1 buffers [PIPE_PW][PIPE_A1R][16] |
                                     // their signal strips [PIPE_PW][PIPE_SG] | conv1 weights [16][K1] | bias [16] | conv3's bias [c3]
    __host__ __device__ PipeLds(int K1, int K3, int s3, int c3) {
        const ConvSpan sp(256, s3, K3, 16);
        span_pos = sp.pos, span_halves = sp.halves;
        xin_halves = (span_halves + 7) & ~7;
        a1 = 2 * xin_halves * 2;
        sl = a1 + PIPE_PW * PIPE_A1R * 16 * 2;
        wl = sl + PIPE_PW * PIPE_SG * 4;
        bl = wl + 16 * K1 * 4;
        b3 = bl + 16 * 4;
        bytes = b3 + c3 * 4;
    }
};

template <int FPW, int NKS>
__global__ __launch_bounds__(64 * (PIPE_CW + PIPE_PW)) void conv_front3_pipe_kernel(ConvFront3Args q, int nb, int total) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ConvArgs& p = q.c3;
    constexpr int PB = 256, C16 = 16, NT = 64 * (PIPE_CW + PIPE_PW);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, kg = lane >> 4;
    const PipeLds L(q.K1, p.K, p.stride, C16 * FPW * PIPE_CW);
    const int span_pos = L.span_pos, span_halves = L.span_halves, xin_halves = L.xin_halves;
    half_t* xin0 = (half_t*)smem;
    half_t* a1all = (half_t*)(smem + L.a1);
    float* slall = (float*)(smem + L.sl);
    float* wl = (float*)(smem + L.wl);
    float* bl = (float*)(smem + L.bl);
    float* b3l = (float*)(smem + L.b3);                               // zeros without a bias

    // this workgroup's run of (chunk, block) pairs
    const int first = (int)((long)blockIdx.x * total / gridDim.x);
    const int nrun = (int)((long)(blockIdx.x + 1) * total / gridDim.x) - first;

    for (int i = tid; i < C16 * q.K1; i += NT) wl[i] = q.w1[i];
    if (tid < C16) bl[tid] = q.b1 ? q.b1[tid] : 0.0f;
    for (int i = tid; i < C16 * FPW * PIPE_CW; i += NT) b3l[i] = p.bias ? p.bias[i] : 0.0f;
    for (int b = 0; b < 2; ++b)
        for (int e = span_pos * C16 + tid; e < span_halves; e += NT) xin0[b * xin_halves + e] = (half_t)0.0f;   // tails read by conv3's zero-padded k columns
    for (int e = tid; e < PIPE_PW * PIPE_A1R * C16; e += NT) a1all[e] = (half_t)0.0f;    // rows under conv2's zero-padded k columns: never anything but finite values
    __syncthreads();

    if (wave >= PIPE_CW) {
        // ---- producers: signal -> conv1 -> conv2 -> span buffer it & 1 ------------------------------------------------------------
        // One producer shares its SIMD with two consumers, and it is the youngest of the three: at equal priority it gets the issue slots
        // the consumers leave, finishes its block behind them and the barrier waits for it (2048 x 10000: 1.50 ms; with the producers
        // at priority 1 1.31, the consumers taking what is left of a SIMD they cannot fill alone)
        __builtin_amdgcn_s_setprio(1);
        const int pw = wave - PIPE_CW;
        half_t* a1 = a1all + pw * PIPE_A1R * C16;
        float* sl = slall + pw * PIPE_SG;
        half8_t a2[3];
        float b2v[4];
        conv2_load(a2, b2v, q.w2pk, q.b2, q.K2, r, kg);
        const int c0t = (lane & 1) * 8;
        float w1r[8][5], w1b[8];
        if (q.K1 == 5) conv1_load5(w1r, w1b, wl, bl, c0t);
        const int halo = q.K2 - 1;
        half_t sv[PIPE_NSV];
        auto fetch = [&](const half_t* sg, int s0, int len) {             // samples s0 + lane, s0 + lane + 64 of the chunk, zero outside it
#pragma unroll
            for (int u = 0; u < PIPE_NSV; ++u) {
                const int i = lane + 64 * u, pos = s0 + i;
                sv[u] = (half_t)0.0f;
                if (i < len && pos >= 0 && pos < q.L0) sv[u] = sg[pos];
            }
        };
        __builtin_amdgcn_s_waitcnt(0x0F70);                               // vmcnt(0): conv2's fragments have landed; inside the loop only samples are in flight
        for (int it = 0; it <= nrun; ++it) {
            if (it < nrun) {
                const int item = first + it, n = item / nb, t0 = (item - n * nb) * PB;
                half_t* xin = xin0 + (it & 1) * xin_halves;
                const int p3_start = t0 * p.stride - p.pad;               // conv2 position of span row 0
                const int vt = min(PB, (p.Lout - t0 + 15) & ~15);         // positions of this block's tiles
                const int rows = min(span_pos, (vt - 1) * p.stride + 2 * NKS);   // span rows they read
                const int ntl = (rows + 15) >> 4;
                const int tlo = ntl * pw / PIPE_PW, thi = ntl * (pw + 1) / PIPE_PW;   // this wave's tiles
                const half_t* sg = q.sig + (long)n * q.L0;
                for (int ts = tlo; ts < thi; ts += PIPE_SL / 16) {
                    const int nt = min(PIPE_SL / 16, thi - ts);
                    const int r0 = ts * 16;                               // span row of the slice's first conv2 row
                    // a1 row i = conv1 position u0 + i; its first tap = signal position s0 + i = strip element i
                    const int u0 = p3_start + r0 - q.pad2, s0 = u0 - q.pad1;
                    const bool head = ts == tlo;
                    wave_lds_sync();                                      // the previous slice's reads of the strip and of a1 are issued
                    // the strip (at most PIPE_SG - 4 samples, two per lane): the head slice fetches its own, every other slice finds
                    // its samples in registers, requested one slice earlier
                    if (head) fetch(sg, s0, nt * 16 + halo + q.K1 - 1);
#pragma unroll
                    for (int u = 0; u < PIPE_NSV; ++u)
                        if (lane + 64 * u < nt * 16 + halo + q.K1 - 1) sl[lane + 64 * u] = (float)sv[u];
                    if (ts + PIPE_SL / 16 < thi) fetch(sg, s0 + PIPE_SL, min(PIPE_SL / 16, thi - ts - PIPE_SL / 16) * 16 + halo + q.K1 - 1);
                    if (!head && lane < 2 * halo)                         // the halo rows: the last K2 - 1 conv1 rows of the previous (full) slice
                        *(half8_t*)(a1 + lane * 8) = *(const half8_t*)(a1 + PIPE_SL * C16 + lane * 8);
                    wave_lds_sync();
                    const int i_lo = head ? 0 : halo, i_hi = nt * 16 + halo;
                    // conv1 of the slice: eight channels (c0t) of one position per item, as conv_front3_kernel
                    conv1_rows<true, 64>(a1, sl, u0, 2 * i_lo + lane, 2 * i_hi, c0t, w1r, w1b, wl, bl, q);
                    wave_lds_sync();
                    // conv2 of the slice's tiles
#pragma unroll
                    for (int tt = 0; tt < PIPE_SL / 16; ++tt)
                        if (tt < nt) conv2_tile<true>(a2, b2v, a1 + (tt * 16 + r) * C16 + kg * 8, xin, r0 + tt * 16 + r, p3_start, span_pos, kg, q);
                }
            }
            __syncthreads();
        }
    } else {
        // ---- consumers: conv3 (conv_ws_kernel's block) on span buffer (it - 1) & 1 --------------------------------------------------
        half8_t afr[FPW][NKS];
        ws_load_fragments(afr, p, wave, r, kg);
        const int RS = p.stride * C16;
        // the fragments have landed before the loop: a wait for them inside it would also wait, block after block, for the output stores
        // (loads and stores share one in-order counter)
        __builtin_amdgcn_s_waitcnt(0x0F70);                                   // vmcnt(0)
        for (int it = 0; it <= nrun; ++it) {
            if (it >= 1) {
                const int item = first + it - 1, n = item / nb, t0 = (item - n * nb) * PB;
                const half_t* xin = xin0 + ((it - 1) & 1) * xin_halves;
                // the lane's row and k-group are derived again for every block: held across the loop, the addresses made of them are
                // spilled (the weight fragments leave no register), and a reload from scratch waits for the block's output stores
                int ln;
                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
                const int r = ln & 15, kg = ln >> 4;
                ws_block<FPW, NKS, true, 1>(afr, WsBiasLds<FPW>{b3l, wave, kg}, xin, RS, p, n, t0, wave, r, kg);
            }
            __syncthreads();
        }
    }
}

}  // namespace bh

// bh_k_conv_last_kernel (test hook, not thread-safe): the bh_conv_kernel code of the last convolution launch of this process
static int g_conv_last_kernel = 0;
void bh_k_conv_note_kernel(int code) { g_conv_last_kernel = code; }
int bh_k_conv_last_kernel() { return g_conv_last_kernel; }

// ---- the instances and their launcher ---------------------------------------------------------------------------------------------
namespace {
using namespace bh;
using ConvKernel = void (*)(ConvArgs);
using Front3Kernel = void (*)(ConvFront3Args);
using PipeKernel = void (*)(ConvFront3Args, int, int);

struct IgemmInstance { int ntt; bool fs; ConvKernel fn; int code; };       // 64 * ntt positions per workgroup
#define BH_IGEMM_ROW(NTT, FS) {NTT, FS, conv_igemm_kernel<NTT, FS>, BH_CONV_K_IGEMM(NTT, FS ? 1 : 0)}
const IgemmInstance IGEMM_INSTANCES[] = {BH_IGEMM_ROW(4, false), BH_IGEMM_ROW(2, false), BH_IGEMM_ROW(1, false),
                                         BH_IGEMM_ROW(4, true),  BH_IGEMM_ROW(2, true),  BH_IGEMM_ROW(1, true)};
#undef BH_IGEMM_ROW

// the two weight-stationary geometries (conv3 of hac-sized and of fast-sized models): feature tiles per wave, k-steps, waves
struct WsInstance { int cout, threads; ConvKernel ws; Front3Kernel front3; PipeKernel pipe; int ws_code, front3_code; };
const WsInstance WS_INSTANCES[] = {
    {384, 512, conv_ws_kernel<3, 10, 8>, conv_front3_kernel<3, 10, 8>, conv_front3_pipe_kernel<3, 10>, BH_CONV_K_WS_384, BH_CONV_K_FRONT3_384},
    {96, 384, conv_ws_kernel<1, 10, 6>, conv_front3_kernel<1, 10, 6>, nullptr, BH_CONV_K_WS_96, BH_CONV_K_FRONT3_96},
};
const WsInstance* ws_instance(int cout) {
    for (const WsInstance& w : WS_INSTANCES)
        if (w.cout == cout) return &w;
    return nullptr;
}

// every launch of this file: the LDS limit of the kernel raised where the caller's rule says so, the launch, its error, the test hook
template <class... A>
int conv_launch(void (*fn)(A...), dim3 grid, dim3 block, size_t lds, bool raise_lds, hipStream_t stream, int code, const A&... args) {
    if (raise_lds) BH_CHECK_HIP(bh_max_lds((const void*)fn, (int)lds));
    hipLaunchKernelGGL(fn, grid, block, lds, stream, args...);
    BH_CHECK_HIP(hipGetLastError());
    g_conv_last_kernel = code;
    return 0;
}
}  // namespace

int bh_k_conv_first(const void* signal, const float* w, const float* bias, void* out, int N, int Lin,
                    int Lout, int Cout, int K, int stride, int pad, int act, float clamp_lo,
                    float clamp_hi, long os_n, long os_t, hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(K >= 1 && Cout >= 1, "conv_first: bad shape (K=%d Cout=%d)", K, Cout);
    const int vec8 = (Cout % 8 == 0 && os_t % 8 == 0 && os_n % 8 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    ConvFirstArgs a{(const half_t*)signal, w, bias, (half_t*)out, N, Lin, Lout, Cout, K, stride, pad,
                    act, clamp_lo, clamp_hi, os_n, os_t, vec8};
    size_t lds = (size_t)(Cout * K + Cout + 255 * stride + K) * sizeof(float);
    return conv_launch(conv_first_kernel, dim3((Lout + 255) / 256, N), dim3(256), lds, false, stream, BH_CONV_K_FIRST, a);
}

// bh::g_opt (options.h), as this file reads it:
// conv_ws 0: always the generic implicit-GEMM kernel (A/B, regression tests)
// conv_fuse 0: the three separate kernels instead of conv_front3_kernel (A/B, regression tests)
// conv_front_pipe 0: conv_front3_kernel<3, 10, 8> instead of conv_front3_pipe_kernel for the 384-channel stacks (A/B, byte reference)
// conv_front_wgs: cap of conv_front3_pipe_kernel's grid (0: one workgroup per CU; tests use it to make a workgroup walk several blocks of a small shape)
// conv_fs 0: never the feature-split instance of conv_igemm_kernel (A/B, tests)
// conv_lds_kb: LDS a workgroup of conv_igemm_kernel may take for its input span; the positions per
                        // workgroup follow. Measured on the v5 sup model (256 x 12000, conv class per batch): position-split instances
                        // 3.85 ms at 64 KiB, 3.25 at 80, 3.68 at 104, 4.28 at 150 (one workgroup per CU); with four k-steps of weight
                        // fragments per trip 2.99 at 80; feature-split instances (FS) 2.4-2.6 anywhere from 24 to 64 KiB, 2.69 at 80
int bh_k_conv_igemm(const void* in, const void* wpk, const float* bias, void* out, int N, int Lin,
                    int Lout, int Cin, int Cout, int K, int stride, int pad, int act, float clamp_lo,
                    float clamp_hi, long os_n, long os_t, hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(Cin % 8 == 0 && Cout % 4 == 0, "conv_igemm: need Cin%%8==0, Cout%%4==0 (Cin=%d Cout=%d)", Cin, Cout);
    BH_REQUIRE(os_t % 4 == 0 && os_n % 4 == 0, "conv_igemm: output strides must be multiples of 4");
    ConvArgs a{(const half_t*)in, (const half_t*)wpk, bias, (half_t*)out, N, Lin, Lout, Cin, Cout, K,
               stride, pad, act, ((K * Cin + 31) / 32) * 32, clamp_lo, clamp_hi, os_n, os_t};
    auto lds_for = [&](int pw) { return ConvSpan(4 * pw, stride, K, Cin).bytes(); };     // pw positions per wave, four waves
    // wide output layer with the k-step count of the bonito conv3 (19 taps x 16 channels): weight-stationary kernel. It loads four
    // biases at a time (float4), so a bias that is not 16-byte aligned goes to the generic kernel, which reads them one by one
    const WsInstance* wsi = ws_instance(Cout);
    if (bh::g_opt.conv_ws && wsi && a.Kp == 320 && lds_for(64) <= 64 * 1024 && ((uintptr_t)bias & 15) == 0)
        return conv_launch(wsi->ws, dim3((Lout + 255) / 256, N), dim3(wsi->threads), lds_for(64), false, stream, wsi->ws_code, a);
    int pw = 64;
    while (pw > 16 && lds_for(pw) > (size_t)bh::g_opt.conv_lds_kb * 1024) pw >>= 1;
    const size_t lds = lds_for(pw);
    BH_REQUIRE(lds <= 160 * 1024, "conv_igemm: input span does not fit LDS (%zu bytes)", lds);
    const bool fs = bh::g_opt.conv_fs && Cout % 64 == 0;
    for (const IgemmInstance& k : IGEMM_INSTANCES)
        if (k.ntt == pw / 16 && k.fs == fs)
            return conv_launch(k.fn, dim3((Lout + 4 * pw - 1) / (4 * pw), N), dim3(256), lds, lds > 64 * 1024, stream, k.code, a);
    BH_REQUIRE(false, "conv_igemm: no instance for %d positions per wave, fs=%d", pw, (int)fs);
}


// Can the three convolutions at the head of an LSTM model run as conv_front3_kernel? Three questions, asked separately:
//  * bh_k_conv_front3_shape_ok: what the KERNEL needs of the arguments its launcher takes. K1 <= 8 (conv1's taps; the signal span is sized for
//    them), K2 * 16 <= 96 (conv2's three k-steps), conv3 what conv_ws_kernel serves (384 / 96 channels, padded K3 * 16 == 320: ten k-steps
//    held in registers), and a workgroup's LDS within 80 KiB. The launcher requires it; nothing else protects the packed weights from
//    being read outside.
//  * bh_k_conv_front3_option_ok: the process-wide options ("conv_fuse", "conv_ws").
//  * bh_k_conv_front3_ok: the engine's question - channel counts as laid out (16 everywhere between the layers), strides 1 in front of
//    conv3, and both of the above.
static int conv_front3_kp(int K3) { return ((K3 * 16 + 31) / 32) * 32; }
int bh_k_conv_front3_shape_ok(int K1, int K2, int c3_out, int K3, int s3) {
    if (K1 < 1 || K1 > 8 || K2 < 1 || K2 * 16 > 96 || K3 < 1 || s3 < 1) return 0;
    if (!ws_instance(c3_out) || conv_front3_kp(K3) != 320) return 0;
    if (s3 > 64) return 0;      // far beyond 80 KiB (stride 10 is); keeps the layout's int arithmetic in range
    return bh::Front3Lds(K1, K2, K3, s3).bytes <= 80 * 1024 ? 1 : 0;
}
int bh_k_conv_front3_option_ok(int c3_out) {
    if (!bh::g_opt.conv_fuse || !bh::g_opt.conv_ws) return 0;
    // 96 channels (the fast models): correct (tests run it with "conv_fuse" 2) but not the default - those models keep three batches in
    // flight whose recurrent kernels share the CUs with the convolutions, and the 65 KiB, 384-thread fused workgroups cost that
    // pipeline more than the 0.04 ms of convolution time they save (bench step 2.43 -> 2.55-2.65 ms)
    return (c3_out == 96 && bh::g_opt.conv_fuse < 2) ? 0 : 1;
}
int bh_k_conv_front3_ok(int c1_eff, int K1, int s1, int c2_in_eff, int c2_eff, int K2, int s2, int c3_in_eff, int c3_out, int K3, int s3) {
    if (c1_eff != 16 || c2_in_eff != 16 || c2_eff != 16 || c3_in_eff != 16 || s1 != 1 || s2 != 1) return 0;
    return bh_k_conv_front3_shape_ok(K1, K2, c3_out, K3, s3) && bh_k_conv_front3_option_ok(c3_out);
}

int bh_k_conv_front3(const void* signal, int N, int L0, const float* w1, const float* b1, int K1, int pad1, int act1, float lo1, float hi1,
                     const void* w2pk, const float* b2, int K2, int pad2, int act2, float lo2, float hi2, const void* w3pk,
                     const float* b3, int Cout3, int K3, int stride3, int pad3, int act3, float lo3, float hi3, void* out, long os_n,
                     long os_t, hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(bh_k_conv_front3_shape_ok(K1, K2, Cout3, K3, stride3),
               "conv_front3: no instance for K1=%d K2=%d Cout3=%d K3=%d stride3=%d (bh_k_conv_front3_shape_ok)", K1, K2, Cout3, K3, stride3);
    BH_REQUIRE(((uintptr_t)b3 & 15) == 0, "conv_front3: conv3's bias must be 16-byte aligned (or null)");
    const int L1 = L0 + 2 * pad1 - K1 + 1, L2 = L1 + 2 * pad2 - K2 + 1, L3 = (L2 + 2 * pad3 - K3) / stride3 + 1;
    BH_REQUIRE(L1 > 0 && L2 > 0 && L3 > 0, "conv_front3: chunk of %d samples is too short", L0);
    BH_REQUIRE(os_t % 4 == 0 && os_n % 4 == 0, "conv_front3: output strides must be multiples of 4");
    ConvFront3Args a{(const half_t*)signal, w1, b1, (const half_t*)w2pk, b2, L0, L1, L2, K1, pad1, act1, K2, pad2, act2, lo1, hi1, lo2, hi2,
                     ConvArgs{nullptr, (const half_t*)w3pk, b3, (half_t*)out, N, L2, L3, 16, Cout3, K3, stride3, pad3, act3, conv_front3_kp(K3), lo3, hi3,
                              os_n, os_t}};
    const WsInstance& wsi = *ws_instance(Cout3);       // (the shape predicate found it)
    const int nb = (L3 + 255) / 256;
    if (wsi.pipe && bh::g_opt.conv_front_pipe) {
        // the pipelined instance: a persistent grid of at most one workgroup per CU, each with a contiguous run of the N * nb blocks
        const long total = (long)N * nb;
        BH_REQUIRE(total < (1l << 30), "conv_front3: %ld blocks are more than the pipelined kernel indexes", total);
        long wgs = bh_cu_count() > 0 ? bh_cu_count() : 256;
        if (bh::g_opt.conv_front_wgs > 0 && bh::g_opt.conv_front_wgs < wgs) wgs = bh::g_opt.conv_front_wgs;
        if (wgs > total) wgs = total;
        return conv_launch(wsi.pipe, dim3((unsigned)wgs), dim3(64 * (PIPE_CW + PIPE_PW)), (size_t)PipeLds(K1, K3, stride3, Cout3).bytes, true, stream,
                           wsi.front3_code, a, nb, (int)total);
    }
    const size_t lds = (size_t)Front3Lds(K1, K2, K3, stride3).bytes;
    return conv_launch(wsi.front3, dim3(nb, N), dim3(wsi.threads), lds, lds > 64 * 1024, stream, wsi.front3_code, a);
}
