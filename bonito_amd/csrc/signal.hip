// Signal ingest on the device: raw int16 ADC samples -> pA -> normalisation -> adapter trim -> fp16 chunk rows of
// the encoder's input batch. Replaces the per-read numpy work of the reference's bonito/pod5.py:57-67 with bonito/reader.py:
// 122-166 (`normalisation`, `trim`) under it, plus `util.chunk` + the fp16 cast of crf/basecall.py:33 for the product path: the
// host ships 2 bytes per sample once and a table of chunk origins.
//
// Everything here reproduces the reference's arithmetic bit for bit. tests/test_gpu_signal.py holds shift / scale (fp64 bits),
// trim and every fp16 chunk sample to tests/signal_ref.py, a line-by-line restatement that tests/golden/signal_cases.npz pins to
// the reference itself; the cases include every int16 value under both strategies.
//   scaled  = f32(scaling) * (f32(raw) + f32(offset))                       two fp32 roundings, no fma
//   quantile strategy:
//     qa, qb  = np.quantile(scaled, [a, b])    order statistics are taken on the raw int16 values (the map to pA is
//               monotone for scaling > 0), interpolation as numpy's _lerp: diff in fp32, the rest in fp64
//     shift   = max(10, m_shift * (qa + qb)), scale = max(1.0, m_scale * (qb - qa))    fp64; Python's max() returns the
//               int 10 / the float 1.0 themselves when they win: Python scalars, where the others are np.float64
//   fixed pA strategy: shift, scale = the config's mean, stdev (or 0.0, 1.0): Python scalars both
//   NumPy's promotion rules (NEP 50) decide the rest. A Python scalar is rounded to the array's fp32 and the operation stays
//   in fp32; a np.float64 takes it to fp64. The per-read `weak` word records which is which:
//     bit 0  shift is Python's 10          bit 1  scale is Python's 1.0          bit 2  fixed pA: both are Python floats
//   thresh  = scale * 2.4 + shift              fp64, two roundings; a Python float only when shift and scale both are
//   trim    : `scaled > thresh` on the pA signal, in fp32 against f32(thresh) for a Python float, in fp64 otherwise
//   norm    = (scaled - shift) / scale          fp32 subtract / divide with the constants rounded to fp32, or fp64
//   chunk rows = f16(f32(norm))                 round-to-nearest-even twice, as torch casts fp64 to fp16 on the CPU
#include "common.h"
#include "kernels.h"

// Every fp operation in this file is one IEEE operation of the reference's NumPy code: build.py compiles it with
// -ffp-contract=off (HIP's __fmul_rn / __fsub_rn are plain operators and WOULD be contracted under the default
// -ffp-contract=fast, which also ignores `#pragma clang fp contract`: cs*xb - cs*xa became fma(cs, xb, -(cs*xa)), i.e.
// the rounding error of the product instead of 0).

namespace bh {

struct SigStatsArgs {
    const int16_t* raw;      // concatenated reads
    const long* offs;        // [R+1] sample offsets
    const float* cal_scale;  // [R]
    const float* cal_offset; // [R]
    int R;
    double qa, qb, shift_mult, scale_mult;
    int strategy;            // 0 quantile, 1 fixed pA (shift/scale given), see bh_signal_normalise
    double fixed_shift, fixed_scale;
    double* shift;           // [R]
    double* scale;           // [R]
    int* weak;               // [R] WEAK_SHIFT | WEAK_SCALE | WEAK_FIXED
    int* trim;               // [R]
    int do_trim, window, min_trim, min_elements, max_samples;
    double threshold, max_trim;     // threshold: in units of scale above shift (2.4)
};

__device__ __forceinline__ float to_pa(int16_t raw, float cs, float co) { return __fmul_rn(cs, __fadd_rn((float)raw, co)); }

enum { WEAK_SHIFT = 1, WEAK_SCALE = 2, WEAK_FIXED = 4 };      // bits of the per-read `weak` word, see the head of the file

// norm = (scaled - shift) / scale under NumPy's promotion rules, rounded to fp32
__device__ __forceinline__ float normalise(float scaled, double shift, double scale, int weak) {
    if (weak & WEAK_FIXED) return __fdiv_rn(__fsub_rn(scaled, (float)shift), (float)scale);
    if ((weak & 3) == 3) return __fsub_rn(scaled, 10.0f);                                  // / 1.0f is exact
    if (weak & WEAK_SHIFT) return (float)((double)__fsub_rn(scaled, 10.0f) / scale);
    return (float)(((double)scaled - shift) / scale);                                      // a weak 1.0 divides exactly
}
// the trim threshold on the pA signal and whether it is a Python float (bonito/pod5.py:62)
__device__ __forceinline__ double trim_threshold(double shift, double scale, double mult) { return scale * mult + shift; }
__device__ __forceinline__ bool threshold_is_weak(int weak) { return (weak & WEAK_FIXED) || (weak & 3) == 3; }
__device__ __forceinline__ bool above_threshold(float scaled, double thr, bool thr_weak) {
    return thr_weak ? scaled > (float)thr : (double)scaled > thr;
}

// k-th smallest (0-based) of the read's int16 values: 256-bin histogram of the high byte, then of the low byte inside the
// selected bin. One workgroup per read; hist = 256 ints of LDS.
__device__ int select_rank(const int16_t* x, long n, long k, int* hist, int* pick) {
    const int tid = threadIdx.x;
    for (int pass = 0; pass < 2; ++pass) {
        hist[tid] = 0;
        __syncthreads();
        const int hi_sel = pick[0];
        for (long i = tid; i < n; i += blockDim.x) {
            const unsigned u = (unsigned)((int)x[i] + 32768);
            if (pass == 0) atomicAdd(&hist[u >> 8], 1);
            else if ((int)(u >> 8) == hi_sel) atomicAdd(&hist[u & 255], 1);
        }
        __syncthreads();
        if (tid == 0) {
            long below = pass == 0 ? 0 : (long)pick[1] | ((long)pick[2] << 31);     // samples below the selected high bin
            int b = 0;
            for (; b < 255; ++b) {
                if (below + hist[b] > k) break;
                below += hist[b];
            }
            if (pass == 0) { pick[0] = b; pick[1] = (int)(below & 0x7fffffff); pick[2] = (int)(below >> 31); }
            else pick[3] = b;
        }
        __syncthreads();
    }
    return ((pick[0] << 8) | pick[3]) - 32768;
}

__device__ double np_lerp(float a, float b, double t) {      // numpy/lib/_function_base_impl.py::_lerp on float32 data
    const float diff = __fsub_rn(b, a);
    return t >= 0.5 ? (double)b - (double)diff * (1.0 - t) : (double)a + (double)diff * t;
}

__global__ __launch_bounds__(256) void signal_stats_kernel(SigStatsArgs p) {
    __shared__ int hist[256];
    __shared__ int pick[4];
    __shared__ int s_trim;
    const int r = blockIdx.x;
    const long o0 = p.offs[r], n = p.offs[r + 1] - o0;
    const int16_t* x = p.raw + o0;
    const float cs = p.cal_scale[r], co = p.cal_offset[r];
    double shift = p.fixed_shift, scale = p.fixed_scale;
    int weak = WEAK_FIXED;
    if (p.strategy == 0) {
        weak = 0;
        double q[2];
        for (int which = 0; which < 2; ++which) {
            const double vi = (double)(n - 1) * (which == 0 ? p.qa : p.qb);
            const long prev = (long)floor(vi);
            const long next = prev + 1 < n ? prev + 1 : n - 1;
            const double gamma = vi - (double)prev;
            const int a = select_rank(x, n, prev, hist, pick);
            const int b = next == prev ? a : select_rank(x, n, next, hist, pick);
            q[which] = np_lerp(to_pa((int16_t)a, cs, co), to_pa((int16_t)b, cs, co), gamma);

        }
        const double sh = p.shift_mult * (q[0] + q[1]), sc = p.scale_mult * (q[1] - q[0]);
        if (sh > 10.0) shift = sh; else { shift = 10.0; weak |= WEAK_SHIFT; }        // max(10, x): the first argument wins ties
        if (sc > 1.0) scale = sc; else { scale = 1.0; weak |= WEAK_SCALE; }
    }
    if (threadIdx.x == 0) { p.shift[r] = shift; p.scale[r] = scale; p.weak[r] = weak; s_trim = 0; }
    __syncthreads();
    // ---- adapter trim (reader.py trim): sequential over windows, one wave, lanes = samples of the window ------------
    if (p.do_trim && threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const long limit = n < p.max_samples ? n : p.max_samples;
        const double thr = trim_threshold(shift, scale, p.threshold);
        const bool thr_weak = threshold_is_weak(weak);
        bool seen = false;
        int result = p.min_trim;
        const int nwin = (int)(limit / p.window);
        for (int pos = 0; pos < nwin; ++pos) {
            const long start = (long)pos * p.window + p.min_trim, end = start + p.window;
            int cnt = 0;
            bool last_above = false;
            for (int base = 0; base < p.window; base += 64) {
                const long i = start + base + lane;
                bool above = false;
                if (base + lane < p.window && i < n) above = above_threshold(to_pa(x[i], cs, co), thr, thr_weak);
                cnt += __popcll(__ballot(above));
                // window[-1]: the last element that exists (numpy slicing clips at the end of the signal)
                const long last = (end < n ? end : n) - 1;
                if (i == last && last >= start) last_above = above;
            }
            last_above = __any(last_above);
            const bool empty = start >= n;            // an empty window: count 0, window[-1] raises in numpy -> cannot happen
            if (seen || cnt > p.min_elements) {
                seen = true;
                if (!empty && last_above) continue;
                if (end >= limit || (double)end / (double)n > p.max_trim) { result = p.min_trim; break; }
                result = (int)end;
                break;
            }
        }
        if (lane == 0) s_trim = result;
    }
    __syncthreads();
    if (threadIdx.x == 0) p.trim[r] = p.do_trim ? s_trim : 0;
}

struct SigChunkArgs {
    const int16_t* raw;
    const long* offs;
    const float* cal_scale;
    const float* cal_offset;
    const double* shift;
    const double* scale;
    const int* weak;
    const int* chunk_read;   // [n_chunks] read index
    const long* chunk_start; // [n_chunks] first sample of the chunk inside the read (trim already added by the caller)
    const long* chunk_len;   // [n_chunks] samples available from chunk_start (>= L for a plain chunk; shorter: tile, util.chunk)
    int n_chunks, L;
    half_t* out;             // [n_chunks][L]
};

__global__ __launch_bounds__(256) void signal_chunk_kernel(SigChunkArgs p) {
    const int cidx = blockIdx.y;
    const int r = p.chunk_read[cidx];
    const int16_t* x = p.raw + p.offs[r] + p.chunk_start[cidx];
    const long len = p.chunk_len[cidx];
    const float cs = p.cal_scale[r], co = p.cal_offset[r];
    const double shift = p.shift[r], scale = p.scale[r];
    const int weak = p.weak[r];
    half_t* o = p.out + (long)cidx * p.L;
    // 4 samples per thread: rows are 8-byte aligned whenever L % 4 == 0 (the usual chunk sizes are multiples of the model
    // stride times 2, e.g. 9996), otherwise element-wise stores
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= p.L) return;
    half4_t v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long i = i0 + e;
        const long src = len >= p.L ? i : i % len;            // short read: tiled to fill the chunk (util.chunk)
        v[e] = i < p.L ? (half_t)normalise(to_pa(x[src], cs, co), shift, scale, weak) : (half_t)0;
    }
    if ((p.L & 3) == 0) *(half4_t*)(o + i0) = v;
    else
        for (int e = 0; e < 4 && i0 + e < p.L; ++e) o[i0 + e] = v[e];
}

}  // namespace bh

int bh_k_signal_normalise(const int16_t* raw, const long* offs, const float* cal_scale, const float* cal_offset, int R,
                          int strategy, double qa, double qb, double shift_mult, double scale_mult, double fixed_shift,
                          double fixed_scale, int do_trim, double* shift, double* scale, int* weak, int* trim, hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(R > 0 && raw && offs && cal_scale && cal_offset && shift && scale && weak && trim, "signal_normalise: bad arguments");
    BH_REQUIRE(strategy == 0 || strategy == 1, "signal_normalise: strategy must be 0 (quantile) or 1 (fixed)");
    SigStatsArgs a{raw, offs, cal_scale, cal_offset, R, qa, qb, shift_mult, scale_mult, strategy, fixed_shift, fixed_scale,
                   shift, scale, weak, trim, do_trim, 40, 10, 3, 8000, 2.4, 0.3};
    hipLaunchKernelGGL(signal_stats_kernel, dim3(R), dim3(256), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}

int bh_k_signal_chunks(const int16_t* raw, const long* offs, const float* cal_scale, const float* cal_offset, const double* shift,
                       const double* scale, const int* weak, const int* chunk_read, const long* chunk_start, const long* chunk_len,
                       int n_chunks, int L, void* out, hipStream_t stream) {
    using namespace bh;
    BH_REQUIRE(n_chunks > 0 && L > 0, "signal_chunks: need n_chunks > 0 and a positive chunk length");
    SigChunkArgs a{raw, offs, cal_scale, cal_offset, shift, scale, weak, chunk_read, chunk_start, chunk_len, n_chunks, L, (half_t*)out};
    hipLaunchKernelGGL(signal_chunk_kernel, dim3(((L + 3) / 4 + 255) / 256, n_chunks), dim3(256), 0, stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return 0;
}
