// What the block-per-workgroup attention kernels share, stated once: attention_kernel (attention.hip: inference, and with LSE the training
// forward) and the two backward passes attn_bwd_q_kernel / attn_bwd_kv_kernel (attention_train.hip). The backward recomputes exp(s - lse)
// and is right only while that is the forward's probability to within the rounding of one fp16 element: the staging layouts, the rotary
// arithmetic and the two tile products are these functions in all three kernels. (One site does not call load_pieces: the forward's Q
// load, see there. hipcc contracts a*co - b*si per call site, so "the same expression" is the same to an fp16 ulp, not to the bit.)
//
// Geometry: a workgroup = 8 waves = (chunk, head, QB consecutive rows of one operand); wave w owns rows 16 w .. 16 w + 15 of the block in
// registers and meets NT tiles of 16 staged rows of the other operand, the first of them staged row 16 w. Staged rows live in LDS either
// row-major ([rows][128 B], 16-byte chunks XOR-swizzled by row & 7: conflict-free fragment reads) or transposed ([64][stride] halves).
#pragma once
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace bh {

constexpr int QB = 128;          // rows per workgroup: queries (forward, query pass) or keys (key pass)
constexpr int HD = 64;           // head_dim
constexpr int THREADS = 512;
constexpr float QK_SCALE = 0.125f;      // 1 / sqrt(HD): on the rotated q before its one rounding to fp16, and on dq

// NT = tiles (of 16 staged rows) per wave, even. The last wave's first tile starts at staged row 7 * 16.
constexpr int staged_rows(int NT) { return 7 * 16 + NT * 16; }
constexpr int t_stride(int NT) { return staged_rows(NT) + 4; }          // halves per feature row of a transposed region (4 of padding)
constexpr size_t rows_bytes(int NT) { return (size_t)staged_rows(NT) * 128; }
constexpr size_t cols_bytes(int NT) { return (size_t)HD * t_stride(NT) * 2; }
constexpr size_t lds_forward(int NT) { return rows_bytes(NT) + cols_bytes(NT); }           // K rows | V^T
constexpr size_t lds_query_pass(int NT) { return rows_bytes(NT) + cols_bytes(NT); }        // K rows | V rows, then K^T over them
constexpr size_t lds_key_pass(int NT) { return 2 * cols_bytes(NT) + 2 * staged_rows(NT) * sizeof(float); }      // Q rows then Q^T | dO rows then dO^T | lse | delta
static_assert(cols_bytes(6) >= rows_bytes(6), "a transposed region also holds the same rows row-major");

// 64 features of one row as the two 8-wide pieces (x1 = dims c*8.., x2 = dims 32 + c*8..) a lane or a staging task handles; ROT: rotary by the
// row's angles (cs_row: the row's 32 (cos, sin) pairs), each element rounded to fp16 once (SCALED: times `scale` before that rounding)
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

// the same rows transposed -> dst [64][VS] halves (feature-major); a task = (row pair, piece): two adjacent rows make the stores 4 bytes
template <bool ROT, bool SCALED>
__device__ __forceinline__ void stage_cols(half_t* dst, int VS, const half_t* src, long stride, int first, int KR, int T, const float* cs, float scale) {
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

// one score-like tile: sum over the 64 features of (staged row `row` = tile start + lane & 15) x (the lane's register fragment f0 | f1). In the
// accumulator a lane (g = lane >> 4) then holds staged rows tile start + 4 g .. + 3 of ONE register row
__device__ __forceinline__ float4_t row_tile(const char* rows, int row, int g, half8_t f0, half8_t f1) {
    const char* rp = rows + row * 128;
    const half8_t a0 = *(const half8_t*)(rp + ((g ^ (row & 7)) << 4));
    const half8_t a1 = *(const half8_t*)(rp + (((g + 4) ^ (row & 7)) << 4));
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
    acc = mfma16(a0, f0, acc);
    acc = mfma16(a1, f1, acc);
    return acc;
}

// o[mt] += X^T (features mt*16 .. x staged rows kcol .. kcol + 3 and kcol + 16 .. + 19: this lane's share of two row tiles) times the B
// fragment pb, whose halves are the two tiles' accumulator-layout values: the contraction order is permuted identically in A and B
__device__ __forceinline__ void col_step(const half_t* xt, int VS, int kcol, int lane, half8_t pb, float4_t (&o)[4]) {
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

// four fp32 values rounded to fp16 (to nearest) and held PACKED in two registers: a tile's share of a B fragment. The empty asm pins the
// packed value HERE: the fragments are used behind a barrier and a staging loop, and the compiler otherwise sinks the exponentials, the
// products and the conversions down to that use, keeping eight fp32 registers per tile alive instead of two (it spilled from NT = 18 on).
// The backward passes only: the forward has no barrier between its softmax and its product and forms its fragments where it uses them.
__device__ __forceinline__ uint2_t pack4(float a, float b, float c, float d) {
    const half4_t h = {(half_t)a, (half_t)b, (half_t)c, (half_t)d};
    uint2_t u = __builtin_bit_cast(uint2_t, h);
    asm volatile("" : "+v"(u.x), "+v"(u.y));
    return u;
}

// o[mt] += X^T (the wave's staged rows r0 ..) times the packed fragments b[kt] of its NT row tiles
template <int NT>
__device__ __forceinline__ void col_product(const half_t* xt, int VS, int r0, int lane, const uint2_t (&b)[NT], float4_t (&o)[4]) {
#pragma unroll
    for (int c = 0; c < NT / 2; ++c) {
        const half8_t pb = __builtin_bit_cast(half8_t, uint4_t{b[2 * c].x, b[2 * c].y, b[2 * c + 1].x, b[2 * c + 1].y});
        col_step(xt, VS, r0 + c * 32 + (lane >> 4) * 4, lane, pb, o);
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

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// The rung ladder: launch(std::integral_constant<int, NT>) -> int for the smallest instance whose NT tiles cover what one wave can see
// under the window. Instances exist for these four NT and no others; the top rung is BH_ATTN_MAX_TILES (kernels.h).
template <class F>
inline int attn_for_rung(int win_left, int win_right, F&& launch) {
    const long need = bh_k_attention_tiles(win_left, win_right);
    if (need <= 6) return launch(std::integral_constant<int, 6>{});
    if (need <= 10) return launch(std::integral_constant<int, 10>{});
    if (need <= 18) return launch(std::integral_constant<int, 18>{});
    if (need <= BH_ATTN_MAX_TILES) return launch(std::integral_constant<int, BH_ATTN_MAX_TILES>{});
    bh_set_error("attention: no kernel instance for %ld tiles per wave", need);          // attn_block_check refuses these first
    return -2;
}

// the grids are (blocks of QB, nhead, N): y and z are limited to 65535
inline bool attn_block_grid_ok(int N, int T, int nhead) { return N >= 1 && T >= 1 && nhead >= 1 && N <= 65535 && nhead <= 65535; }

// The problems the block kernels serve; `what` is the entry's name in the messages. Every entry calls it in front of its first launch.
inline int attn_block_check(const char* what, int N, int T, int nhead, int head_dim, int win_left, int win_right) {
    BH_REQUIRE(head_dim == HD, "%s: only head_dim 64 is implemented (got %d)", what, head_dim);
    BH_REQUIRE(win_left >= 0 && win_right >= 0, "%s: a finite window (left, right) is required (got (%d, %d))", what, win_left, win_right);
    BH_REQUIRE(bh_k_attention_serves(win_left, win_right), "%s: window %d+%d is too wide for the LDS-resident kernels", what, win_left, win_right);
    BH_REQUIRE(attn_block_grid_ok(N, T, nhead), "%s: N, T and nhead must be positive, N and nhead at most 65535 (got N=%d T=%d nhead=%d)", what, N, T,
               nhead);
    return 0;
}

// launch of a block kernel with its dynamic LDS bytes (the limit is raised where a rung needs more than 64 KiB)
template <class Args>
inline int attn_block_launch(void (*kernel)(Args), size_t lds, dim3 grid, hipStream_t stream, const Args& args) {
    if (lds > 64 * 1024) BH_CHECK_HIP(bh_max_lds((const void*)kernel, (int)lds));
    hipLaunchKernelGGL(kernel, grid, dim3(THREADS), lds, stream, args);
    return 0;
}

}  // namespace bh
