// Rotary embedding + sliding-window attention on packed qkv for TRAINING on gfx950 (head_dim 64): the forward that keeps what the
// backward needs, and the backward. The arithmetic is stated in include/bonito_hip.h under bh_attention_train_forward.
//
// Forward: attention_kernel<NT, true> of attention.hip - the inference kernel, instantiated to also write lse = m + ln(sum) of every
// query's softmax row (fp32 [N][H][T], the `saved` buffer). `out` has the bytes of bh_attention.
//
// Backward: no atomics and no order that depends on scheduling - with a sliding window two passes give every gradient row ONE owner.
// Both recompute S from LDS-staged operands with the MFMAs of the forward (so exp(s - lse) is the forward's probability):
//   delta pass  delta_i = sum_d dO_id O_id (fp32, O the stored fp16 output) into the workspace, [N][H][T].
//   query pass  workgroup = 8 waves = (chunk, head, 128 queries), the forward's geometry: the <= 128 + wl + wr keys the block sees are staged
//               row-major (K rotated, V as it is; 16-byte chunks XOR-swizzled by row & 7). A wave owns 16 queries; per key tile of 16 it forms
//               S^T = K Q^T and dP^T = V dO^T (A from LDS, B = the query's fragments in registers) and keeps dS^T = P (dP - delta) as fp16 -
//               in the accumulator layout that IS the B fragment of dQ^T = K^T dS^T. The V region is then overwritten by K^T (the forward's V^T
//               layout) and the wave finishes dQ^T, rotates it back and scales it.
//   key pass    workgroup = (chunk, head, 128 keys): the same geometry with the window mirrored - key j is seen by the queries
//               i in [j - wr, j + wl] - and the roles exchanged: Q (rotated, scaled) and dO are staged, k and v are the register fragments.
//               P and dS are kept as fp16 B fragments; the two regions are then overwritten by Q^T and dO^T for dK^T = Q^T dS, dV^T = dO^T P.
// Chunks and heads never meet: a chunk's bytes do not depend on the rest of the batch.
#include "common.h"
#include "kernels.h"

namespace bh {
namespace {

constexpr int QB = 128;     // queries (query pass) or keys (key pass) per workgroup
constexpr int HD = 64;
constexpr int THREADS = 512;

struct AttnBwdArgs {
    const half_t* qkv;    // [N*T][3*D], q | k | v, head-major inside each
    const float* cs;      // [T][32][2]  (cos, sin) of position * inv_freq
    const half_t* dout;   // [N*T][D]
    const float* lse;     // [N][H][T]
    const float* delta;   // [N][H][T]
    half_t* dqkv;         // [N*T][3*D]
    int N, T, H;
    int wl, wr;           // window: i - wl <= j <= i + wr
};

// 64 features of one row as the two 8-wide pieces (x1 = dims c*8.., x2 = dims 32 + c*8..) a lane or a staging task handles; ROT: rotary by the
// row's angles, each element rounded to fp16 once (SCALED: times `scale` before that rounding). The expressions are those of attention_kernel.
template <bool ROT, bool SCALED>
__device__ __forceinline__ void load_pieces(const half_t* row, const float* cs_row, int c, float scale, half8_t& lo, half8_t& hi) {
    const half8_t x1 = *(const half8_t*)(row + c * 8);
    const half8_t x2 = *(const half8_t*)(row + 32 + c * 8);
    if constexpr (ROT) {
        const float* cs = cs_row + c * 8 * 2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float co = cs[2 * e], si = cs[2 * e + 1];
            const float a = (float)x1[e], b = (float)x2[e];
            if constexpr (SCALED) {
                lo[e] = (half_t)((a * co - b * si) * scale);
                hi[e] = (half_t)((a * si + b * co) * scale);
            } else {
                lo[e] = (half_t)(a * co - b * si);
                hi[e] = (half_t)(a * si + b * co);
            }
        }
    } else {
        lo = x1;
        hi = x2;
    }
}

// rows first .. first + KR - 1 of a matrix (row t at src + t * stride, 64 features) -> dst [KR][128 B], swizzled; rows outside [0, T) are zeros
template <bool ROT, bool SCALED>
__device__ __forceinline__ void stage_rows(char* dst, const half_t* src, long stride, int first, int KR, int T, const float* cs, float scale) {
    for (int task = threadIdx.x; task < KR * 4; task += THREADS) {
        const int r = task >> 2, c = task & 3;
        const int t = first + r;
        half8_t lo = {0, 0, 0, 0, 0, 0, 0, 0}, hi = lo;
        if (t >= 0 && t < T) load_pieces<ROT, SCALED>(src + (long)t * stride, cs + (long)t * 64, c, scale, lo, hi);
        *(half8_t*)(dst + r * 128 + ((c ^ (r & 7)) << 4)) = lo;
        *(half8_t*)(dst + r * 128 + (((c + 4) ^ (r & 7)) << 4)) = hi;
    }
}

// the same rows transposed -> dst [64][VS] halves (feature-major, the V^T layout of attention_kernel); a task = (row pair, piece)
template <bool ROT, bool SCALED>
__device__ __forceinline__ void stage_cols(half_t* dst, int VS, const half_t* src, long stride, int first, int KR, int T, const float* cs,
                                           float scale) {
    for (int task = threadIdx.x; task < (KR / 2) * 4; task += THREADS) {
        const int r = (task >> 2) * 2, c = task & 3;
        half8_t lo[2], hi[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = first + r + u;
            lo[u] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
            hi[u] = lo[u];
            if (t >= 0 && t < T) load_pieces<ROT, SCALED>(src + (long)t * stride, cs + (long)t * 64, c, scale, lo[u], hi[u]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const half2_t pl = {lo[0][e], lo[1][e]}, ph = {hi[0][e], hi[1][e]};
            *(half2_t*)(dst + (c * 8 + e) * VS + r) = pl;
            *(half2_t*)(dst + (32 + c * 8 + e) * VS + r) = ph;
        }
    }
}

// one score-like tile: sum over the 64 features of (staged row r0 + lane & 15) x (the lane's register fragment)
__device__ __forceinline__ float4_t row_tile(const char* rows, int row, int g, const half8_t (&f)[2]) {
    const char* rp = rows + row * 128;
    const half8_t a0 = *(const half8_t*)(rp + ((g ^ (row & 7)) << 4));
    const half8_t a1 = *(const half8_t*)(rp + (((g + 4) ^ (row & 7)) << 4));
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
    acc = mfma16(a0, f[0], acc);
    acc = mfma16(a1, f[1], acc);
    return acc;
}

// four fp32 values rounded to fp16 (to nearest) and held PACKED in two registers: a tile's share of a B fragment. The empty asm pins the
// packed value HERE: the fragments are used behind a barrier and a staging loop, and the compiler otherwise sinks the exponentials, the
// products and the conversions down to that use, keeping eight fp32 registers per tile alive instead of two (it spilled from NT = 18 on).
__device__ __forceinline__ uint2_t pack4(float a, float b, float c, float d) {
    const half4_t h = {(half_t)a, (half_t)b, (half_t)c, (half_t)d};
    uint2_t u = __builtin_bit_cast(uint2_t, h);
    asm volatile("" : "+v"(u.x), "+v"(u.y));
    return u;
}

// o[mt] += X^T (features mt*16.. x the wave's staged rows r0 ..) times the fp16 B fragments b[c] (two row tiles each): attention_kernel's PV loop
template <int NT>
__device__ __forceinline__ void col_product(const half_t* xt, int VS, int r0, int lane, const uint2_t (&b)[NT], float4_t (&o)[4]) {
    const int g = lane >> 4;
#pragma unroll
    for (int c = 0; c < NT / 2; ++c) {
        const half8_t pb = __builtin_bit_cast(half8_t, uint4_t{b[2 * c].x, b[2 * c].y, b[2 * c + 1].x, b[2 * c + 1].y});
        const int kcol = r0 + c * 32 + g * 4;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const half_t* vp = xt + (mt * 16 + (lane & 15)) * VS + kcol;
            const half4_t va = *(const half4_t*)vp;
            const half4_t vb = *(const half4_t*)(vp + 16);
            half8_t af;
#pragma unroll
            for (int e = 0; e < 4; ++e) { af[e] = va[e]; af[4 + e] = vb[e]; }
            o[mt] = mfma16(af, pb, o[mt]);
        }
    }
}

// the lane holds features mt*16 + g*4 + e of one row's rotated gradient in o[mt][e]: rotate back by the row's angles (the pair of feature d < 32
// is d + 32 = o[mt + 2]), scale, round once, store
__device__ __forceinline__ void store_unrotated(half_t* dst, const float4_t (&o)[4], const float* cs_row, int g, float scale) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        half4_t x1, x2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = mt * 16 + g * 4 + e;
            const float co = cs_row[2 * d], si = cs_row[2 * d + 1];
            const float a = o[mt][e], b = o[mt + 2][e];
            x1[e] = (half_t)((a * co + b * si) * scale);
            x2[e] = (half_t)((b * co - a * si) * scale);
        }
        *(half4_t*)(dst + mt * 16 + g * 4) = x1;
        *(half4_t*)(dst + 32 + mt * 16 + g * 4) = x2;
    }
}

__global__ __launch_bounds__(256) void attn_delta_kernel(const half_t* out, const half_t* dout, float* delta, int N, int T, int H) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * T * H) return;
    const int h = (int)(idx % H);
    const long row = idx / H;
    const half_t* o = out + row * H * HD + h * HD;
    const half_t* d = dout + row * H * HD + h * HD;
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const half8_t ov = *(const half8_t*)(o + c * 8), dv = *(const half8_t*)(d + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += (float)dv[e] * (float)ov[e];
    }
    const long n = row / T, t = row % T;
    delta[(n * H + h) * T + t] = acc;
}

template <int NT>           // key tiles (of 16) per wave, even
__global__ __launch_bounds__(THREADS) void attn_bwd_q_kernel(AttnBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KR = 7 * 16 + NT * 16;          // staged key rows
    constexpr int VS = KR + 4;
    char* kl = smem;                              // [KR][128 B] rotated K
    char* second = smem + KR * 128;               // [KR][128 B] V, then [64][VS] rotated K^T
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = p.H * HD;
    const int h = blockIdx.y, n = blockIdx.z;
    const int i0 = blockIdx.x * QB;
    const int jbase = i0 - p.wl;                  // staged row r <-> key jbase + r
    const half_t* base = p.qkv + (long)n * p.T * 3 * D + h * HD;
    stage_rows<true, false>(kl, base + D, 3 * D, jbase, KR, p.T, p.cs, 1.0f);
    stage_rows<false, false>(second, base + 2 * D, 3 * D, jbase, KR, p.T, p.cs, 1.0f);

    const int qi = i0 + wave * 16 + (lane & 15);
    const int g = lane >> 4;
    half8_t qf[2] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
    half8_t dof[2] = {qf[0], qf[0]};
    float lse = 0.0f, delta = 0.0f;
    if (qi < p.T) {
        load_pieces<true, true>(base + (long)qi * 3 * D, p.cs + (long)qi * 64, g, 0.125f, qf[0], qf[1]);
        load_pieces<false, false>(p.dout + ((long)n * p.T + qi) * D + h * HD, p.cs, g, 1.0f, dof[0], dof[1]);
        lse = p.lse[((long)n * p.H + h) * p.T + qi];
        delta = p.delta[((long)n * p.H + h) * p.T + qi];
    }
    __syncthreads();

    const int r0 = wave * 16;
    uint2_t ds[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        const int row = r0 + kt * 16 + (lane & 15);
        const float4_t s = row_tile(kl, row, g, qf);
        const float4_t dp = row_tile(second, row, g, dof);
        float dsv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = jbase + r0 + kt * 16 + g * 4 + e;
            const bool ok = j >= 0 && j < p.T && j >= qi - p.wl && j <= qi + p.wr;
            const float x = s[e] - lse;
            const float pv = __expf(ok ? x : -INFINITY);          // exp(-inf) = 0 for masked keys
            dsv[e] = pv * (dp[e] - delta);
        }
        ds[kt] = pack4(dsv[0], dsv[1], dsv[2], dsv[3]);
    }
    __syncthreads();                              // everybody has read V
    half_t* kt_ = (half_t*)second;
    stage_cols<true, false>(kt_, VS, base + D, 3 * D, jbase, KR, p.T, p.cs, 1.0f);
    __syncthreads();

    float4_t o[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) o[mt] = float4_t{0.f, 0.f, 0.f, 0.f};
    col_product<NT>(kt_, VS, r0, lane, ds, o);
    if (qi < p.T) store_unrotated(p.dqkv + ((long)n * p.T + qi) * 3 * D + h * HD, o, p.cs + (long)qi * 64, g, 0.125f);
}

template <int NT>           // query tiles (of 16) per wave, even
__global__ __launch_bounds__(THREADS) void attn_bwd_kv_kernel(AttnBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KR = 7 * 16 + NT * 16;          // staged query rows
    constexpr int VS = KR + 4;
    constexpr int REGION = 64 * VS * 2;           // bytes: [KR][128 B] rows first, [64][VS] halves afterwards
    char* first = smem;                           // rotated, scaled Q, then its transpose
    char* second = smem + REGION;                 // dO, then its transpose
    float* lse_s = (float*)(smem + 2 * REGION);   // [KR]
    float* delta_s = lse_s + KR;                  // [KR]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = p.H * HD;
    const int h = blockIdx.y, n = blockIdx.z;
    const int j0 = blockIdx.x * QB;
    const int ibase = j0 - p.wr;                  // staged row r <-> query ibase + r: key j is seen by the queries j - wr .. j + wl
    const half_t* base = p.qkv + (long)n * p.T * 3 * D + h * HD;
    const half_t* dob = p.dout + (long)n * p.T * D + h * HD;
    stage_rows<true, true>(first, base, 3 * D, ibase, KR, p.T, p.cs, 0.125f);
    stage_rows<false, false>(second, dob, D, ibase, KR, p.T, p.cs, 1.0f);
    for (int r = tid; r < KR; r += THREADS) {
        const int i = ibase + r;
        const bool in = i >= 0 && i < p.T;
        lse_s[r] = in ? p.lse[((long)n * p.H + h) * p.T + i] : 0.0f;
        delta_s[r] = in ? p.delta[((long)n * p.H + h) * p.T + i] : 0.0f;
    }

    const int kj = j0 + wave * 16 + (lane & 15);
    const int g = lane >> 4;
    half8_t kf[2] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
    half8_t vf[2] = {kf[0], kf[0]};
    if (kj < p.T) {
        load_pieces<true, false>(base + (long)kj * 3 * D + D, p.cs + (long)kj * 64, g, 1.0f, kf[0], kf[1]);
        load_pieces<false, false>(base + (long)kj * 3 * D + 2 * D, p.cs, g, 1.0f, vf[0], vf[1]);
    }
    __syncthreads();

    const int r0 = wave * 16;
    uint2_t pr[NT], ds[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        const int row = r0 + kt * 16 + (lane & 15);
        const float4_t s = row_tile(first, row, g, kf);
        const float4_t dp = row_tile(second, row, g, vf);
        const int rq = r0 + kt * 16 + g * 4;      // this lane's four query rows of the tile
        const float4_t lse4 = *(const float4_t*)(lse_s + rq), delta4 = *(const float4_t*)(delta_s + rq);
        float pv[4], dsv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = ibase + rq + e;
            const bool ok = i >= 0 && i < p.T && i >= kj - p.wr && i <= kj + p.wl && kj < p.T;
            const float x = s[e] - lse4[e];
            pv[e] = __expf(ok ? x : -INFINITY);          // exp(-inf) = 0 for queries that do not see the key
            dsv[e] = pv[e] * (dp[e] - delta4[e]);
        }
        pr[kt] = pack4(pv[0], pv[1], pv[2], pv[3]);
        ds[kt] = pack4(dsv[0], dsv[1], dsv[2], dsv[3]);
    }
    __syncthreads();                              // everybody has read the rows
    stage_cols<true, true>((half_t*)first, VS, base, 3 * D, ibase, KR, p.T, p.cs, 0.125f);
    stage_cols<false, false>((half_t*)second, VS, dob, D, ibase, KR, p.T, p.cs, 1.0f);
    __syncthreads();

    float4_t ok_[4], ov[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        ok_[mt] = float4_t{0.f, 0.f, 0.f, 0.f};
        ov[mt] = float4_t{0.f, 0.f, 0.f, 0.f};
    }
    col_product<NT>((const half_t*)second, VS, r0, lane, pr, ov);
    col_product<NT>((const half_t*)first, VS, r0, lane, ds, ok_);
    if (kj < p.T) {
        half_t* dst = p.dqkv + ((long)n * p.T + kj) * 3 * D + h * HD;
        store_unrotated(dst + D, ok_, p.cs + (long)kj * 64, g, 1.0f);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            half4_t x;
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = (half_t)ov[mt][e];
            *(half4_t*)(dst + 2 * D + mt * 16 + g * 4) = x;
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool problem_ok(int N, int T, int nhead) { return N >= 1 && T >= 1 && nhead >= 1 && N <= 65535 && nhead <= 65535; }
inline size_t stat_bytes(int N, int T, int nhead) { return align_up256((size_t)N * nhead * T * sizeof(float)); }

}  // namespace
}  // namespace bh

size_t bh_k_attention_train_saved_bytes(int N, int T, int nhead) { return bh::problem_ok(N, T, nhead) ? bh::stat_bytes(N, T, nhead) : 0; }
size_t bh_k_attention_train_backward_workspace(int N, int T, int nhead, int win_left, int win_right) {
    return bh::problem_ok(N, T, nhead) && bh_k_attention_serves(win_left, win_right) ? bh::stat_bytes(N, T, nhead) : 0;
}

#define ATTN_TRAIN_SHAPE(what)                                                                                                       \
    BH_REQUIRE(head_dim == 64, what ": only head_dim 64 is implemented (got %d)", head_dim);                                         \
    BH_REQUIRE(win_left >= 0 && win_right >= 0, what ": a finite window (left, right) is required (got (%d, %d))", win_left, win_right); \
    BH_REQUIRE(bh_k_attention_serves(win_left, win_right), what ": window %d+%d is too wide for the LDS-resident kernels", win_left, win_right); \
    BH_REQUIRE(N >= 1 && T >= 1 && nhead >= 1, what ": N, T and nhead must be positive (got N=%d T=%d nhead=%d)", N, T, nhead);      \
    BH_REQUIRE(N <= 65535 && nhead <= 65535, what ": at most 65535 chunks and heads per call (got N=%d nhead=%d)", N, nhead)

int bh_k_attention_train_forward(const void* qkv, const float* cos_sin, int N, int T, int nhead, int head_dim, int win_left, int win_right,
                                 void* out, void* saved, size_t saved_bytes, hipStream_t stream) {
    using namespace bh;
    ATTN_TRAIN_SHAPE("attention_train_forward");
    BH_REQUIRE(qkv && cos_sin && out && saved, "attention_train_forward: null pointer");
    BH_REQUIRE(aligned16(qkv) && aligned16(cos_sin) && aligned16(out) && aligned16(saved),
               "attention_train_forward: qkv, cos_sin, out and saved must be 16-byte aligned");
    const size_t need = stat_bytes(N, T, nhead);
    BH_REQUIRE(saved_bytes >= need, "attention_train_forward: saved buffer of %zu bytes, bh_attention_train_saved_bytes(%d, %d, %d) = %zu",
               saved_bytes, N, T, nhead, need);
    return bh_k_attention_lse(qkv, out, cos_sin, N, T, nhead, head_dim, win_left, win_right, (float*)saved, stream);
}

int bh_k_attention_train_backward(const void* qkv, const float* cos_sin, const void* out, const void* saved, const void* dout, int N, int T,
                                  int nhead, int head_dim, int win_left, int win_right, void* dqkv, void* workspace, size_t workspace_bytes,
                                  hipStream_t stream) {
    using namespace bh;
    ATTN_TRAIN_SHAPE("attention_train_backward");
    BH_REQUIRE(qkv && cos_sin && out && saved && dout && dqkv && workspace, "attention_train_backward: null pointer");
    BH_REQUIRE(aligned16(qkv) && aligned16(cos_sin) && aligned16(out) && aligned16(saved) && aligned16(dout) && aligned16(dqkv) &&
                   aligned16(workspace),
               "attention_train_backward: qkv, cos_sin, out, saved, dout, dqkv and workspace must be 16-byte aligned");
    const size_t need_ws = stat_bytes(N, T, nhead);
    BH_REQUIRE(workspace_bytes >= need_ws,
               "attention_train_backward: workspace of %zu bytes, bh_attention_train_backward_workspace(%d, %d, %d, %d, %d) = %zu",
               workspace_bytes, N, T, nhead, win_left, win_right, need_ws);
    float* delta = (float*)workspace;
    const long stats = (long)N * T * nhead;
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((stats + 255) / 256)), dim3(256), 0, stream, (const half_t*)out, (const half_t*)dout,
                       delta, N, T, nhead);
    AttnBwdArgs a{(const half_t*)qkv, cos_sin, (const half_t*)dout, (const float*)saved, delta, (half_t*)dqkv, N, T, nhead, win_left, win_right};
    const dim3 grid((T + QB - 1) / QB, nhead, N);
    const int need = (16 + win_left + win_right + 15) / 16;      // tiles one wave can see, in either pass
#define BH_ATTN_BWD(NT)                                                                                          \
    do {                                                                                                         \
        constexpr int KR = 7 * 16 + NT * 16, VS = KR + 4;                                                        \
        const size_t lds_q = (size_t)KR * 128 + (size_t)64 * VS * 2;                                             \
        const size_t lds_kv = (size_t)2 * 64 * VS * 2 + (size_t)2 * KR * sizeof(float);                          \
        if (lds_q > 64 * 1024) BH_CHECK_HIP(bh_max_lds((const void*)attn_bwd_q_kernel<NT>, (int)lds_q));         \
        if (lds_kv > 64 * 1024) BH_CHECK_HIP(bh_max_lds((const void*)attn_bwd_kv_kernel<NT>, (int)lds_kv));      \
        hipLaunchKernelGGL(attn_bwd_q_kernel<NT>, grid, dim3(THREADS), lds_q, stream, a);                        \
        hipLaunchKernelGGL(attn_bwd_kv_kernel<NT>, grid, dim3(THREADS), lds_kv, stream, a);                      \
    } while (0)
    if (need <= 6) BH_ATTN_BWD(6);
    else if (need <= 10) BH_ATTN_BWD(10);
    else if (need <= 18) BH_ATTN_BWD(18);
    else BH_ATTN_BWD(26);
#undef BH_ATTN_BWD
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
