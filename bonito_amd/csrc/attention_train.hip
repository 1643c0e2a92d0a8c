// Rotary embedding + sliding-window attention on packed qkv for TRAINING on gfx950 (head_dim 64): the forward that keeps what the
// backward needs, and the backward. The arithmetic is stated in include/bonito_hip.h under bh_attention_train_forward.
//
// Forward: attention_kernel<NT, true> of attention.hip - the inference kernel, instantiated to also write lse = m + ln(sum) of every
// query's softmax row (fp32 [N][H][T], the `saved` buffer). `out` has the bytes of bh_attention.
//
// The staging, the fragments, the tile products, the geometry and the rung ladder are attn_block.h's, shared with that kernel.
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
#include "attn_block.h"
#include "common.h"
#include "kernels.h"

namespace bh {
namespace {

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
    constexpr int KR = staged_rows(NT);           // staged key rows
    constexpr int VS = t_stride(NT);
    char* kl = smem;                              // [KR][128 B] rotated K
    char* second = smem + rows_bytes(NT);         // [KR][128 B] V, then [64][VS] rotated K^T
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
        load_pieces<true, true>(base + (long)qi * 3 * D, p.cs + (long)qi * 64, g, QK_SCALE, qf[0], qf[1]);
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
        const float4_t s = row_tile(kl, row, g, qf[0], qf[1]);
        const float4_t dp = row_tile(second, row, g, dof[0], dof[1]);
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
    if (qi < p.T) store_unrotated(p.dqkv + ((long)n * p.T + qi) * 3 * D + h * HD, o, p.cs + (long)qi * 64, g, QK_SCALE);
}

template <int NT>           // query tiles (of 16) per wave, even
__global__ __launch_bounds__(THREADS) void attn_bwd_kv_kernel(AttnBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KR = staged_rows(NT);           // staged query rows
    constexpr int VS = t_stride(NT);
    constexpr int REGION = (int)cols_bytes(NT);   // bytes: [KR][128 B] rows first, [64][VS] halves afterwards
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
    stage_rows<true, true>(first, base, 3 * D, ibase, KR, p.T, p.cs, QK_SCALE);
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
        const float4_t s = row_tile(first, row, g, kf[0], kf[1]);
        const float4_t dp = row_tile(second, row, g, vf[0], vf[1]);
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
    stage_cols<true, true>((half_t*)first, VS, base, 3 * D, ibase, KR, p.T, p.cs, QK_SCALE);
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
inline size_t stat_bytes(int N, int T, int nhead) { return align_up256((size_t)N * nhead * T * sizeof(float)); }

}  // namespace
}  // namespace bh

size_t bh_k_attention_train_saved_bytes(int N, int T, int nhead) { return bh::attn_block_grid_ok(N, T, nhead) ? bh::stat_bytes(N, T, nhead) : 0; }
size_t bh_k_attention_train_backward_workspace(int N, int T, int nhead, int win_left, int win_right) {
    return bh::attn_block_grid_ok(N, T, nhead) && bh_k_attention_serves(win_left, win_right) ? bh::stat_bytes(N, T, nhead) : 0;
}

int bh_k_attention_train_forward(const void* qkv, const float* cos_sin, int N, int T, int nhead, int head_dim, int win_left, int win_right,
                                 void* out, void* saved, size_t saved_bytes, hipStream_t stream) {
    using namespace bh;
    if (const int rc = attn_block_check("attention_train_forward", N, T, nhead, head_dim, win_left, win_right)) return rc;
    BH_REQUIRE(qkv && cos_sin && out && saved, "attention_train_forward: null pointer");
    BH_REQUIRE(aligned16(qkv) && aligned16(cos_sin) && aligned16(out) && aligned16(saved),
               "attention_train_forward: qkv, cos_sin, out and saved must be 16-byte aligned");
    const size_t need = stat_bytes(N, T, nhead);
    BH_REQUIRE(saved_bytes >= need, "attention_train_forward: saved buffer of %zu bytes, bh_attention_train_saved_bytes(%d, %d, %d) = %zu",
               saved_bytes, N, T, nhead, need);
    return bh_k_attention_block(qkv, out, cos_sin, N, T, nhead, win_left, win_right, (float*)saved, stream);
}

int bh_k_attention_train_backward(const void* qkv, const float* cos_sin, const void* out, const void* saved, const void* dout, int N, int T,
                                  int nhead, int head_dim, int win_left, int win_right, void* dqkv, void* workspace, size_t workspace_bytes,
                                  hipStream_t stream) {
    using namespace bh;
    if (const int rc = attn_block_check("attention_train_backward", N, T, nhead, head_dim, win_left, win_right)) return rc;
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
    const int rc = attn_for_rung(win_left, win_right, [&](auto nt) {          // the tiles one wave can see are the same in either pass
        constexpr int NT = decltype(nt)::value;
        if (const int e = attn_block_launch(attn_bwd_q_kernel<NT>, lds_query_pass(NT), grid, stream, a)) return e;
        return attn_block_launch(attn_bwd_kv_kernel<NT>, lds_key_pass(NT), grid, stream, a);
    });
    if (rc != 0) return rc;
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
