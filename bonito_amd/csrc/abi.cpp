// The operator-level extern "C" shells declared in include/bonito_hip.h: argument checks in front of the launchers of kernels.h,
// host-side weight packing, and the process-wide option switch. The encoder (bh_encoder_*) lives in engine.cpp.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/bonito_hip.h"
#include "common.h"
#include "devbuf.h"
#include "kernels.h"
#include "lstm_pack.h"
#include "options.h"

extern "C" size_t bh_conv1d_packed_halves(int Cin, int Cout, int K) {
    size_t kp = ((size_t)K * Cin + 31) / 32 * 32;
    size_t c16 = ((size_t)Cout + 15) / 16 * 16;
    return kp * c16;
}
// torch conv weight [Cout][Cin][K] -> [Cout16][Kp], column index = k*Cin + c (channel-minor taps)
extern "C" int bh_conv1d_pack(const float* w, int Cin, int Cout, int K, uint16_t* packed) {
    BH_REQUIRE(w && packed && Cin > 0 && Cout > 0 && K > 0, "conv1d_pack: bad arguments");
    size_t kp = ((size_t)K * Cin + 31) / 32 * 32;
    size_t c16 = ((size_t)Cout + 15) / 16 * 16;
    memset(packed, 0, kp * c16 * 2);
    for (int f = 0; f < Cout; ++f)
        for (int c = 0; c < Cin; ++c)
            for (int k = 0; k < K; ++k)
                packed[(size_t)f * kp + (size_t)k * Cin + c] = f2h(w[((size_t)f * Cin + c) * K + k]);
    return 0;
}
// W_hh [4H][H] (torch gate order i,f,g,o) -> [slice][gate][kstep][lane][8]: the A fragment of
// mfma 16x16x32 for rows gate*H + slice*16 + (lane&15), k = kstep*32 + (lane>>4)*8 + j.
extern "C" int bh_lstm_pack_whh(const float* whh, int H, uint16_t* packed) {
    BH_REQUIRE(whh && packed && H % 32 == 0 && H > 0, "lstm_pack_whh: H must be a positive multiple of 32");
    const int nks = H / 32, nsl = H / 16;
    for (int s = 0; s < nsl; ++s)
        for (int g = 0; g < 4; ++g)
            for (int ks = 0; ks < nks; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        int row = g * H + s * 16 + (lane & 15);
                        int col = ks * 32 + (lane >> 4) * 8 + j;
                        packed[((((size_t)s * 4 + g) * nks + ks) * 64 + lane) * 8 + j] =
                            f2h(whh[(size_t)row * H + col]);
                    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// operator-level shells
extern "C" int bh_linear(const void* X, const void* W, const float* bias, void* out, int M, int N, int K, int ldx,
                         int ldw, int ldo, int act, float scale, float clamp_lo, float clamp_hi, int gated,
                         int row_div, long row_s_hi, long row_s_lo, int row_lim, void* stream) {
    BH_REQUIRE(X && W && out, "linear: null pointer");
    return bh_k_linear(X, W, bias, out, M, N, K, ldx, ldw, ldo, act, scale, clamp_lo, clamp_hi, gated, row_div,
                       row_s_hi, row_s_lo, row_lim, (hipStream_t)stream);
}
extern "C" int bh_linear_residual(const void* X, const void* W, const float* bias, void* out, int M, int N, int K, int ldx,
                                  int ldw, int ldo, int act, float scale, float clamp_lo, float clamp_hi, int gated,
                                  int row_div, long row_s_hi, long row_s_lo, int row_lim, const void* residual, int ldres,
                                  float res_scale, void* stream) {
    BH_REQUIRE(X && W && out && residual, "linear_residual: null pointer");
    return bh_k_linear(X, W, bias, out, M, N, K, ldx, ldw, ldo, act, scale, clamp_lo, clamp_hi, gated, row_div,
                       row_s_hi, row_s_lo, row_lim, (hipStream_t)stream, residual, ldres, res_scale);
}
extern "C" int bh_linear_qkv_rotary(const void* X, const void* W, const float* bias, void* out, int M, int D, int K,
                                    const float* cos_sin, int T, float qscale, void* stream) {
    BH_REQUIRE(X && W && out && cos_sin, "linear_qkv_rotary: null pointer");
    return bh_k_linear_qkv_rotary(X, W, bias, out, M, D, K, cos_sin, T, qscale, (hipStream_t)stream);
}
extern "C" int bh_linear_last_kernel(void) { return bh_k_linear_last_kernel(); }
extern "C" int bh_conv1d_first(const void* signal, const float* w, const float* bias, void* out, int N, int Lin,
                               int Cout, int K, int stride, int pad, int act, float clamp_lo, float clamp_hi,
                               long os_n, long os_t, void* stream) {
    BH_REQUIRE(signal && w && out && stride > 0, "conv1d_first: bad arguments");
    const int lout = conv_out_len(Lin, K, stride, pad);
    BH_REQUIRE(lout > 0, "conv1d_first: input too short");
    return bh_k_conv_first(signal, w, bias, out, N, Lin, lout, Cout, K, stride, pad, act, clamp_lo, clamp_hi, os_n,
                           os_t, (hipStream_t)stream);
}
extern "C" int bh_conv1d(const void* in, const void* wpacked, const float* bias, void* out, int N, int Lin, int Cin,
                         int Cout, int K, int stride, int pad, int act, float clamp_lo, float clamp_hi, long os_n,
                         long os_t, void* stream) {
    BH_REQUIRE(in && wpacked && out && stride > 0, "conv1d: bad arguments");
    const int lout = conv_out_len(Lin, K, stride, pad);
    BH_REQUIRE(lout > 0, "conv1d: input too short");
    return bh_k_conv_igemm(in, wpacked, bias, out, N, Lin, lout, Cin, Cout, K, stride, pad, act, clamp_lo, clamp_hi,
                           os_n, os_t, (hipStream_t)stream);
}
extern "C" int bh_conv1d_front3(const void* signal, int N, int L0, const float* w1, const float* b1, int K1, int pad1, int act1, float lo1,
                                float hi1, const void* w2packed, const float* b2, int K2, int pad2, int act2, float lo2, float hi2,
                                const void* w3packed, const float* b3, int Cout3, int K3, int stride3, int pad3, int act3, float lo3,
                                float hi3, void* out, long os_n, long os_t, void* stream) {
    BH_REQUIRE(signal && w1 && w2packed && w3packed && out && stride3 > 0 && N > 0, "conv1d_front3: bad arguments");
    BH_REQUIRE(bh_k_conv_front3_shape_ok(K1, K2, Cout3, K3, stride3),
               "conv1d_front3: the fused front end has no instance for K1=%d K2=%d Cout3=%d K3=%d stride3=%d", K1, K2, Cout3, K3, stride3);
    const int l1 = conv_out_len(L0, K1, 1, pad1);
    const int l2 = l1 > 0 ? conv_out_len(l1, K2, 1, pad2) : 0;
    const int l3 = l2 > 0 && l2 + 2 * pad3 >= K3 ? conv_out_len(l2, K3, stride3, pad3) : 0;
    BH_REQUIRE(l1 > 0 && l2 > 0 && l3 > 0, "conv1d_front3: input too short");
    return bh_k_conv_front3(signal, N, L0, w1, b1, K1, pad1, act1, lo1, hi1, w2packed, b2, K2, pad2, act2, lo2, hi2, w3packed, b3, Cout3,
                            K3, stride3, pad3, act3, lo3, hi3, out, os_n, os_t, (hipStream_t)stream);
}
extern "C" int bh_conv1d_last_kernel(void) { return bh_k_conv_last_kernel(); }
// cos/sin of position * 10000^(-2i/dim), interleaved [T][dim/2][2], fp32 products like flash_attn's rotary
extern "C" int bh_rotary_table(int T, int dim, float* out) {
    BH_REQUIRE(out && T > 0 && dim > 0 && dim % 2 == 0, "rotary_table: bad arguments");
    const int half = dim / 2;
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < half; ++i) {
            const float inv = 1.0f / powf(10000.0f, (float)(2 * i) / (float)dim);
            const float ang = (float)t * inv;
            out[((size_t)t * half + i) * 2] = cosf(ang);
            out[((size_t)t * half + i) * 2 + 1] = sinf(ang);
        }
    return 0;
}
extern "C" int bh_attention(const void* qkv, void* out, const float* cos_sin, int N, int T, int nhead, int head_dim,
                            int win_left, int win_right, void* stream) {
    BH_REQUIRE(qkv && out && cos_sin, "attention: null pointer");
    return bh_k_attention(qkv, out, cos_sin, N, T, nhead, head_dim, win_left, win_right, (hipStream_t)stream);
}
extern "C" int bh_attention_prerotated(const void* qkv, void* out, int N, int T, int nhead, int head_dim, int win_left, int win_right,
                                       void* stream) {
    BH_REQUIRE(qkv && out, "attention_prerotated: null pointer");
    return bh_k_attention_prerotated(qkv, out, N, T, nhead, head_dim, win_left, win_right, (hipStream_t)stream);
}
extern "C" int bh_rmsnorm_residual(const void* a, const void* x, const float* w, void* out, long M, int D, float alpha,
                                   float eps, void* stream) {
    BH_REQUIRE(a && w && out && M > 0, "rmsnorm_residual: bad arguments");      // x == NULL: `a` already holds the residual sum
    return bh_k_rmsnorm_residual(a, x, w, out, M, D, alpha, eps, (hipStream_t)stream);
}
extern "C" int bh_ctc_greedy_decode(const float* logp, const long* offsets, int R, int classes, float qscale, float qbias,
                                    int8_t* labels, int8_t* qual, int* path, int* count, void* stream) {
    BH_REQUIRE(logp && offsets && labels && qual && path && count, "ctc_greedy_decode: null pointer");
    return bh_k_ctc_greedy(logp, offsets, R, classes, qscale, qbias, labels, qual, path, count, (hipStream_t)stream);
}
extern "C" size_t bh_ctc_beam_search_workspace(long total_steps, int R, int classes, int beam_size) {
    return bh_k_ctc_beam_workspace(total_steps, R, classes, beam_size);
}
extern "C" int bh_ctc_beam_search(const float* logp, const long* offsets, int R, int classes, int beam_size, float threshold,
                                  void* workspace, int8_t* labels, int* path, int* count, void* stream) {
    BH_REQUIRE(logp && offsets && workspace && labels && path && count, "ctc_beam_search: null pointer");
    return bh_k_ctc_prefix_beam(logp, offsets, R, classes, beam_size, threshold, workspace, labels, path, count,
                                (hipStream_t)stream);
}
extern "C" int bh_dwconv1d(const void* in, const float* w, void* out, int N, int Lin, int C, int K, int stride, int pad,
                           void* stream) {
    BH_REQUIRE(in && w && out && stride > 0, "dwconv1d: bad arguments");
    const int lout = conv_out_len(Lin, K, stride, pad);
    BH_REQUIRE(lout > 0, "dwconv1d: input too short");
    return bh_k_dwconv(in, w, out, N, Lin, lout, C, K, stride, pad, (hipStream_t)stream);
}
extern "C" int bh_ctc_head(const void* in, const float* w, const float* bias, void* out, long M, int features, int classes,
                           void* stream) {
    BH_REQUIRE(in && w && bias && out && M > 0, "ctc_head: bad arguments");
    return bh_k_ctc_head(in, w, bias, out, M, features, classes, (hipStream_t)stream);
}
extern "C" size_t bh_lstm_workspace(int N, int H) { return bh_k_lstm_ws_bytes(N, H); }
extern "C" int bh_lstm_layer(const void* gates_in, const void* whh_packed, void* h_out, int T, int N, int H,
                             int reverse, void* workspace, int* err_flag, int flags, void* stream) {
    BH_REQUIRE(gates_in && whh_packed && h_out && err_flag && workspace, "lstm_layer: null pointer");
    BH_REQUIRE(T > 0, "lstm_layer: T must be positive");
    int rc = bh_k_fill_u16(h_out, 0xFFFFu, (size_t)T * N * H, (hipStream_t)stream);
    if (rc) return rc;
    bh_lstm_launch layer{};
    layer.family = H > 512 || (flags & 2) ? BH_LSTM_STREAM : BH_LSTM_WAVE;     // flags bit 1: force the weight-streaming kernel
    layer.input = gates_in; layer.w_hh = whh_packed; layer.h_out = h_out;
    layer.T = T; layer.N = N; layer.H = H;
    layer.R = layer.n_rings = N / 16;
    layer.reverse = reverse;
    layer.err_flag = err_flag; layer.xcc_ws = (int*)workspace;
    layer.write_through = flags & 1;
    // the streaming kernel's batch is split (at 8 rings even where the device holds fewer: the launch then says so); the
    // register-resident kernel's is one launch
    const bh_lstm_instance* row = bh_k_lstm_find(layer.family, H, 0);
    const int per = layer.family == BH_LSTM_STREAM && row ? std::max(8, row->geo.rings_per_launch(bh_cu_count())) : std::max(1, layer.R);
    return bh_k_lstm_run_layer(layer, per, false, (hipStream_t)stream);
}
// Operator level (parity tests): one Q8-1 recurrent layer straight from fp32 host weights. Packs, uploads, quantises x with
// the static scale 127 / bound, runs the 8-bit kernel and synchronises. `sums` (optional) receives the exact int32 partial sums
// [T][N][4H][2] (input part, recurrent part) the gate arithmetic started from; `hq_frag` (optional) the int8 output in
// fragment order [T][N/16][ceil(H/64)][64][16]. The kernel instance follows from the outputs asked for, as in forward_lstm_q8:
// sums -> <LAST, DBG> (tests only), else h16_out -> <LAST> (the last recurrent layer), else hq_frag alone -> neither (the layers
// before it). max_rings_per_launch > 0 caps the rings of one launch below what the device holds, so that the split loop runs on
// small batches; it never raises the device's figure. bh_lstm_q8_layer is the same call with max_rings_per_launch = 0.
extern "C" int bh_lstm_q8_layer_split(const void* x, float bound, const float* w_ih, const float* w_hh, const float* bias, int T, int N,
                                      int H, int reverse, int variant, void* h16_out, int8_t* hq_frag, int32_t* sums,
                                      int max_rings_per_launch, void* stream_) {
    BH_REQUIRE(x && w_ih && w_hh && T > 0 && N > 0 && N % 16 == 0 && max_rings_per_launch >= 0, "lstm_q8_layer: bad arguments");
    BH_REQUIRE(h16_out || hq_frag, "lstm_q8_layer: neither h16_out nor hq_frag given");
    BH_REQUIRE(h16_out || !sums, "lstm_q8_layer: sums need h16_out (the instance that dumps them also writes the fp16 rows)");
    const int U = bh_k_lstm_q8_units(H, variant);
    BH_REQUIRE(U != 0, "lstm_q8_layer: hidden size %d is not covered by the 8-bit kernel", H);
    hipStream_t st = (hipStream_t)stream_;
    const int R = N / 16;
    const size_t tile = bh_k_lstm_q8_tile_bytes(H), wbytes = (size_t)4 * H * ((H + 63) / 64 * 64);
    std::vector<int8_t> pk(wbytes);
    std::vector<float> s_ih((size_t)4 * H), s_hh((size_t)4 * H), b((size_t)4 * H, 0.0f);
    DevBuf q_wih, q_whh, q_sx, q_sh, q_b, xq, ex, ws, err;
    if (bh_k_lstm_q8_pack(w_ih, H, U, pk.data(), s_ih.data()) || upload(q_wih, pk.data(), pk.size())) return -1;
    if (bh_k_lstm_q8_pack(w_hh, H, U, pk.data(), s_hh.data()) || upload(q_whh, pk.data(), pk.size())) return -1;
    const float xs = (float)((double)bound / 127.0);
    for (int j = 0; j < 4 * H; ++j) { s_ih[j] *= xs; s_hh[j] /= 127.0f; if (bias) b[j] = bias[j]; }
    if (upload_f32(q_sx, s_ih.data(), s_ih.size()) || upload_f32(q_sh, s_hh.data(), s_hh.size()) || upload_f32(q_b, b.data(), b.size())) return -1;
    if (xq.alloc((size_t)T * R * tile) || ex.alloc(4 * (size_t)R * tile) || ws.alloc(bh_k_lstm_ws_bytes(N, 1024)) || err.alloc(sizeof(int))) return -1;
    BH_CHECK_HIP(hipMemsetAsync(err.p, 0, sizeof(int), st));
    int rc = bh_k_quantise_rows(x, xq.p, T, N, H, R, bound, st);
    if (!rc) rc = bh_k_lstm_q8_arm(ex.p, R, H, st);
    if (rc) return rc;
    int per = bh_k_lstm_q8_geometry(H, variant).rings_per_launch(bh_cu_count());
    BH_REQUIRE(per >= 1, "lstm_q8_layer: device has too few CUs for hidden size %d", H);
    if (max_rings_per_launch > 0) per = std::min(per, max_rings_per_launch);
    for (int r0 = 0; r0 < R; r0 += per) {
        const int nr = std::min(per, R - r0);
        rc = bh_k_lstm_layer_q8((const char*)xq.p + (size_t)r0 * tile, q_wih.p, q_whh.p, (const float*)q_sx.p, (const float*)q_sh.p,
                                (const float*)q_b.p, hq_frag ? (char*)hq_frag + (size_t)r0 * tile : nullptr,
                                h16_out ? (char*)h16_out + (size_t)r0 * 16 * H * 2 : nullptr, (char*)ex.p + (size_t)r0 * tile, T, N, H, R, nr, reverse,
                                (int*)err.p, st, (int*)ws.p, 0, variant, sums ? sums + (size_t)r0 * 16 * 4 * H * 2 : nullptr,
                                (unsigned)bh::g_opt.lstm_max_spins);
        if (rc) return rc;
    }
    int flag = 0;
    BH_CHECK_HIP(hipMemcpyAsync(&flag, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    BH_CHECK_HIP(hipStreamSynchronize(st));
    BH_REQUIRE(flag == 0, "lstm_q8_layer: exchange timeout in the recurrent kernel");
    return 0;
}
extern "C" int bh_lstm_q8_layer(const void* x, float bound, const float* w_ih, const float* w_hh, const float* bias, int T, int N,
                                int H, int reverse, int variant, void* h16_out, int8_t* hq_frag, int32_t* sums, void* stream_) {
    return bh_lstm_q8_layer_split(x, bound, w_ih, w_hh, bias, T, N, H, reverse, variant, h16_out, hq_frag, sums, 0, stream_);
}
// Operator level (parity tests): one fp16 recurrent layer on a chosen kernel family from fp32 host weights, packed by the functions
// bh_encoder_create packs with (lstm_pack.h), in the layouts the instance wants, and launched the way forward_lstm launches it.
extern "C" int bh_lstm_layer_family(const void* x, const float* w_ih, const float* w_hh, const float* bias, int T, int N, int H,
                                    int reverse, int family, int flags, void* h_out, void* stream_) {
    BH_REQUIRE(x && w_ih && w_hh && h_out && x != h_out, "lstm_layer_family: null pointer, or x and h_out are one buffer");
    BH_REQUIRE(T > 0 && N > 0 && H > 0, "lstm_layer_family: T, N, H must be positive");
    BH_REQUIRE(family >= BH_LSTM_WAVE && family < BH_LSTM_Q8, "lstm_layer_family: family %d is not an fp16 family (the 8-bit path: bh_lstm_q8_layer)", family);
    const bh_lstm_instance* row = bh_k_lstm_find(family, H, flags & BH_LSTM_V_OUTPUT);
    BH_REQUIRE(bh_k_lstm_serves(family, H), "lstm_layer_family: family %d has no instance for hidden size %d", family, H);
    BH_REQUIRE(row && (flags & ~(BH_LSTM_V_OUTPUT | 1)) == 0, "lstm_layer_family: flags %d not understood by family %d", flags, family);
    BH_REQUIRE(((uintptr_t)h_out & 15) == 0 && ((uintptr_t)x & 15) == 0, "lstm_layer_family: x and h_out must be 16-byte aligned");
    const bh_lstm_geometry& geo = row->geo;
    BH_REQUIRE(N % geo.ring_chunks == 0, "lstm_layer_family: batch %d is no multiple of the family's ring of %d chunks", N, geo.ring_chunks);
    const int R = N / geo.ring_chunks, per = geo.rings_per_launch(bh_cu_count());
    BH_REQUIRE(R <= per, "lstm_layer_family: %d rings, one launch of family %d holds %d at hidden size %d", R, family, per, H);
    hipStream_t st = (hipStream_t)stream_;
    const size_t nw = (size_t)4 * H * H;
    DevBuf d_wih, d_whh, d_b, gates, ex, ws, err;
    std::vector<uint16_t> pk(nw);
    std::vector<float> b((size_t)4 * H);
    lstm_pack_bias(row->w_ih, bias, nullptr, H, b.data());
    if (upload_f32(d_b, b.data(), b.size())) return -1;
    if (lstm_pack(row->w_ih, row->mt, w_ih, H, H, pk.data()) || upload(d_wih, pk.data(), nw * 2)) return -1;
    if (lstm_pack(row->w_hh, row->mt, w_hh, H, H, pk.data()) || upload(d_whh, pk.data(), nw * 2)) return -1;
    if (ws.alloc(bh_k_lstm_ws_bytes(N, 1024)) || err.alloc(sizeof(int))) return -1;
    if (!row->projects && gates.alloc((size_t)T * N * 4 * H * 2 + 256)) return -1;
    if (row->ex_bytes && ex.alloc((size_t)4 * R * row->ex_bytes + 256)) return -1;
    BH_CHECK_HIP(hipMemsetAsync(err.p, 0, sizeof(int), st));
    int rc = 0;
    if (!row->projects) rc = bh_k_linear(x, d_wih.p, (const float*)d_b.p, gates.p, T * N, 4 * H, H, H, H, 4 * H, bh::ACT_NONE, 1.0f, -INFINITY,
                                         INFINITY, 0, 0, 0, 0, 0, st);
    if (!rc && !row->ex_bytes && !geo.unlimited) rc = bh_k_fill_u16(h_out, 0xFFFFu, (size_t)T * N * H, st);      // hand-off through the output tensor
    if (rc) return rc;
    bh_lstm_launch layer{};
    layer.family = (bh_lstm_family)family;
    layer.input = row->projects ? x : gates.p;
    layer.w_ih = d_wih.p; layer.w_hh = d_whh.p; layer.bias = (const float*)d_b.p;
    layer.h_out = h_out;
    layer.ex = ex.p;
    layer.T = T; layer.N = N; layer.H = H;
    layer.R = layer.n_rings = R;
    layer.reverse = reverse;
    layer.err_flag = (int*)err.p; layer.xcc_ws = (int*)ws.p;
    layer.write_through = flags & 1;
    rc = bh_k_lstm_run_layer(layer, per, false, st);
    if (rc) return rc;
    int flag = 0;
    BH_CHECK_HIP(hipMemcpyAsync(&flag, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    BH_CHECK_HIP(hipStreamSynchronize(st));
    BH_REQUIRE(flag == 0, "lstm_layer_family: exchange timeout in the recurrent kernel");
    return 0;
}
extern "C" size_t bh_beam_search_workspace(int N, int T, int state_len) { return bh_k_beam_workspace(N, T, state_len); }
extern "C" int bh_beam_search(const void* scores, int N, int T, int state_len, int beam_width, float beam_cut,
                              float blank_score, float q_scale, float q_offset, void* workspace, int8_t* sequence,
                              int8_t* qstring, int8_t* moves, float* qfloat, void* stream) {
    BH_REQUIRE(scores && workspace && sequence && qstring && moves, "beam_search: null pointer");
    return bh_k_beam_search(scores, N, T, state_len, beam_width, beam_cut, blank_score, q_scale, q_offset, workspace,
                            sequence, qstring, moves, qfloat, (hipStream_t)stream);
}
extern "C" int bh_lstm_launch_plan(int family, int H, int flags, int n_rings, int cu_count, int32_t* out, int n_out) {
    return bh_k_lstm_launch_plan(family, H, flags, n_rings, cu_count, out, n_out);
}
extern "C" int bh_beam_search_plan(int N, int T, int state_len, int cu_count, int debug, int32_t* out, int n_out) {
    return bh_k_beam_search_plan(N, T, state_len, cu_count, debug, out, n_out);
}
extern "C" int bh_crf_reverse_complement(const void* in, void* out, int N, int T, int state_len, int layout_5s,
                                         long stride_n, long stride_t, void* stream) {
    BH_REQUIRE(in && out, "crf_reverse_complement: null pointer");
    return bh_k_crf_revcomp(in, out, N, T, state_len, layout_5s, stride_n, stride_t, (hipStream_t)stream);
}
extern "C" int bh_crf_logz(const void* scores, int N, int T, int state_len, float blank_score, void* workspace,
                           double* logz, void* stream) {
    BH_REQUIRE(scores && workspace && logz, "crf_logz: null pointer");
    return bh_k_crf_logz(scores, N, T, state_len, blank_score, workspace, logz, (hipStream_t)stream);
}
extern "C" size_t bh_crf_seq_workspace(int N, int T, int Lmax, int state_len) {
    return bh_k_crf_seq_workspace(N, T, Lmax, state_len);
}
extern "C" int bh_crf_seq_logz(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score, long stride_n,
                               long stride_t, const void* targets, int Lmax, int target_bytes, const int32_t* target_lengths,
                               void* workspace, float* logz_out, void* stream) {
    BH_REQUIRE(scores && targets && target_lengths && workspace && logz_out, "crf_seq_logz: null pointer");
    return bh_k_crf_seq(scores, N, T, state_len, layout_5s, blank_score, stride_n, stride_t, targets, target_bytes, Lmax,
                        target_lengths, workspace, logz_out, nullptr, 0, (hipStream_t)stream);
}
extern "C" int bh_crf_seq_logz_free(const void* scores, int N, int T, int state_len, float blank_score, long stride_n, long stride_t,
                                    const void* targets, int Lmax, int target_bytes, const int32_t* target_lengths, void* workspace,
                                    float* logz_out, void* stream) {
    BH_REQUIRE(scores && targets && target_lengths && workspace && logz_out, "crf_seq_logz_free: null pointer");
    return bh_k_crf_seq(scores, N, T, state_len, 0, blank_score, stride_n, stride_t, targets, target_bytes, Lmax, target_lengths,
                        workspace, logz_out, nullptr, 2, (hipStream_t)stream);
}
extern "C" int bh_crf_seq_viterbi(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score, long stride_n,
                                  long stride_t, const void* targets, int Lmax, int target_bytes, const int32_t* target_lengths,
                                  void* workspace, int32_t* align_out, float* best_out, void* stream) {
    BH_REQUIRE(scores && targets && target_lengths && workspace && align_out && best_out, "crf_seq_viterbi: null pointer");
    return bh_k_crf_seq(scores, N, T, state_len, layout_5s, blank_score, stride_n, stride_t, targets, target_bytes, Lmax,
                        target_lengths, workspace, best_out, align_out, 1, (hipStream_t)stream);
}
extern "C" int bh_crf_logz_dense(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score, long stride_n,
                                 long stride_t, float* logz_out, void* stream) {
    BH_REQUIRE(scores && logz_out, "crf_logz_dense: null pointer");
    return bh_k_crf_logz_dense(scores, N, T, state_len, layout_5s, blank_score, stride_n, stride_t, logz_out, (hipStream_t)stream);
}
extern "C" size_t bh_crf_seq_grad_workspace(int N, int T, int Lmax, int state_len) {
    return bh_k_crf_seq_grad_workspace(N, T, Lmax, state_len);
}
extern "C" int bh_crf_seq_logz_grad(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score, long stride_n,
                                    long stride_t, const void* targets, int Lmax, int target_bytes, const int32_t* target_lengths,
                                    const float* weight, void* workspace, float* logz_out, void* grad, long g_stride_n,
                                    long g_stride_t, int grad_fp32, int accumulate, void* stream) {
    BH_REQUIRE(scores && targets && target_lengths && workspace && logz_out && grad, "crf_seq_logz_grad: null pointer");
    return bh_k_crf_seq_grad(scores, N, T, state_len, layout_5s, blank_score, stride_n, stride_t, targets, target_bytes, Lmax,
                             target_lengths, weight, workspace, logz_out, grad, g_stride_n, g_stride_t, grad_fp32, accumulate,
                             (hipStream_t)stream);
}
extern "C" size_t bh_crf_logz_dense_grad_workspace(int N, int T, int state_len) {
    return bh_k_crf_logz_dense_grad_workspace(N, T, state_len);
}
extern "C" int bh_crf_logz_dense_grad(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score,
                                      long stride_n, long stride_t, const float* weight, void* workspace, float* logz_out,
                                      void* grad, long g_stride_n, long g_stride_t, int grad_fp32, void* stream) {
    BH_REQUIRE(scores && workspace && logz_out && grad, "crf_logz_dense_grad: null pointer");
    return bh_k_crf_logz_dense_grad(scores, N, T, state_len, layout_5s, blank_score, stride_n, stride_t, weight, workspace,
                                    logz_out, grad, g_stride_n, g_stride_t, grad_fp32, (hipStream_t)stream);
}
extern "C" size_t bh_ctc_loss_workspace(int N, int T, int C, int Lmax) { return bh_k_ctc_loss_workspace(N, T, C, Lmax, 0); }
extern "C" int bh_ctc_loss(const void* log_probs, int logp_fp32, int N, int T, int C, long stride_t, long stride_n, const void* targets,
                           int Lmax, int target_bytes, const int32_t* target_lengths, const float* smooth_w, void* workspace,
                           float* nll_out, float* smooth_out, void* stream) {
    return bh_k_ctc_loss(log_probs, logp_fp32, N, T, C, stride_t, stride_n, targets, target_bytes, Lmax, target_lengths, smooth_w,
                         nullptr, nullptr, workspace, nll_out, smooth_out, nullptr, 0, 0, 0, 0, 0, (hipStream_t)stream);
}
extern "C" size_t bh_ctc_loss_grad_workspace(int N, int T, int C, int Lmax) { return bh_k_ctc_loss_workspace(N, T, C, Lmax, 1); }
extern "C" int bh_ctc_loss_grad(const void* log_probs, int logp_fp32, int N, int T, int C, long stride_t, long stride_n,
                                const void* targets, int Lmax, int target_bytes, const int32_t* target_lengths, const float* smooth_w,
                                const float* weight, const float* smooth_weight, void* workspace, float* nll_out, float* smooth_out,
                                void* grad, long g_stride_t, long g_stride_n, int grad_fp32, int accumulate, void* stream) {
    return bh_k_ctc_loss(log_probs, logp_fp32, N, T, C, stride_t, stride_n, targets, target_bytes, Lmax, target_lengths, smooth_w,
                         weight, smooth_weight, workspace, nll_out, smooth_out, grad, g_stride_t, g_stride_n, grad_fp32, accumulate, 1,
                         (hipStream_t)stream);
}
extern "C" int bh_ctc_loss_last_kernel(void) { return bh_k_ctc_loss_last_kernel(); }
extern "C" size_t bh_lstm_train_saved_bytes(int T, int N, int H) { return bh_k_lstm_train_saved_bytes(T, N, H); }
extern "C" size_t bh_lstm_train_backward_workspace(int T, int N, int H) { return bh_k_lstm_train_backward_workspace(T, N, H); }
extern "C" int bh_lstm_train_workgroups(int N) { return bh_k_lstm_train_workgroups(N); }
extern "C" int bh_lstm_train_forward(const void* x, const float* w_ih, const float* w_hh, const float* bias, int T, int N, int H,
                                     int reverse, void* h_out, void* saved, size_t saved_bytes, void* stream) {
    return bh_k_lstm_train_forward(x, w_ih, w_hh, bias, T, N, H, reverse, h_out, saved, saved_bytes, (hipStream_t)stream);
}
extern "C" int bh_lstm_train_backward(const void* x, const float* w_ih, const float* w_hh, const void* h, const void* saved, const void* dh,
                                      int T, int N, int H, int reverse, void* dx, float* dw_ih, float* dw_hh, float* dbias, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return bh_k_lstm_train_backward(x, w_ih, w_hh, h, saved, dh, T, N, H, reverse, dx, dw_ih, dw_hh, dbias, workspace, workspace_bytes,
                                    (hipStream_t)stream);
}
extern "C" size_t bh_attention_train_saved_bytes(int N, int T, int nhead) { return bh_k_attention_train_saved_bytes(N, T, nhead); }
extern "C" size_t bh_attention_train_backward_workspace(int N, int T, int nhead, int win_left, int win_right) {
    return bh_k_attention_train_backward_workspace(N, T, nhead, win_left, win_right);
}
extern "C" int bh_attention_train_forward(const void* qkv, const float* cos_sin, int N, int T, int nhead, int head_dim, int win_left,
                                          int win_right, void* out, void* saved, size_t saved_bytes, void* stream) {
    return bh_k_attention_train_forward(qkv, cos_sin, N, T, nhead, head_dim, win_left, win_right, out, saved, saved_bytes, (hipStream_t)stream);
}
extern "C" int bh_attention_train_backward(const void* qkv, const float* cos_sin, const void* out, const void* saved, const void* dout, int N,
                                           int T, int nhead, int head_dim, int win_left, int win_right, void* dqkv, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    return bh_k_attention_train_backward(qkv, cos_sin, out, saved, dout, N, T, nhead, head_dim, win_left, win_right, dqkv, workspace,
                                         workspace_bytes, (hipStream_t)stream);
}
extern "C" size_t bh_conv1d_train_workspace(int N, int Lin, int Cin, int Cout, int K, int stride, int pad) {
    return bh_k_conv_train_workspace(N, Lin, Cin, Cout, K, stride, pad);
}
extern "C" int bh_conv1d_train_forward(const void* x, const float* w, const float* bias, int N, int Lin, int Cin, int Cout, int K, int stride,
                                       int pad, int act, float clamp_lo, float clamp_hi, long os_n, long os_t, void* y, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return bh_k_conv_train_forward(x, w, bias, N, Lin, Cin, Cout, K, stride, pad, act, clamp_lo, clamp_hi, os_n, os_t, y, workspace,
                                   workspace_bytes, (hipStream_t)stream);
}
extern "C" int bh_conv1d_train_backward(const void* x, const float* w, const float* bias, const void* y, const void* dy, int N, int Lin, int Cin,
                                        int Cout, int K, int stride, int pad, int act, float clamp_lo, float clamp_hi, long os_n, long os_t,
                                        void* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    return bh_k_conv_train_backward(x, w, bias, y, dy, N, Lin, Cin, Cout, K, stride, pad, act, clamp_lo, clamp_hi, os_n, os_t, dx, dw, db,
                                    workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" size_t bh_linear_train_workspace(int T, int N, int K, int C) { return bh_k_linear_train_workspace(T, N, K, C); }
extern "C" int bh_linear_train_forward(const void* x, const float* w, const float* bias, int T, int N, int K, int C, int act, float scale,
                                       float clamp_lo, float clamp_hi, int batch_major, void* y, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return bh_k_linear_train_forward(x, w, bias, T, N, K, C, act, scale, clamp_lo, clamp_hi, batch_major, y, workspace, workspace_bytes,
                                     (hipStream_t)stream);
}
extern "C" int bh_linear_train_backward(const void* x, const float* w, const void* y, const void* dy, int T, int N, int K, int C, int act,
                                        float scale, float clamp_lo, float clamp_hi, int batch_major, void* dx, float* dw, float* db,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return bh_k_linear_train_backward(x, w, y, dy, T, N, K, C, act, scale, clamp_lo, clamp_hi, batch_major, dx, dw, db, workspace,
                                      workspace_bytes, (hipStream_t)stream);
}
extern "C" size_t bh_rmsnorm_train_workspace(long M, int D) { return bh_k_rmsnorm_train_workspace(M, D); }
extern "C" int bh_rmsnorm_train_backward(const void* a, const void* x, const float* w, const void* dy, long M, int D, float alpha, float eps,
                                         void* da, void* dx, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
    return bh_k_rmsnorm_train_backward(a, x, w, dy, M, D, alpha, eps, da, dx, dw, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" size_t bh_gated_linear_train_workspace(long M, int D, int F) { return bh_k_gated_linear_train_workspace(M, D, F); }
extern "C" int bh_gated_linear_train_forward(const void* x, const float* w, long M, int D, int F, void* h, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    return bh_k_gated_linear_train_forward(x, w, M, D, F, h, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int bh_gated_linear_train_backward(const void* x, const float* w, const void* dh, long M, int D, int F, void* dx, float* dw,
                                              void* workspace, size_t workspace_bytes, void* stream) {
    return bh_k_gated_linear_train_backward(x, w, dh, M, D, F, dx, dw, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" size_t bh_batchnorm_train_workspace(int N, int L, int C) { return bh_k_batchnorm_train_workspace(N, L, C); }
extern "C" int bh_batchnorm_train_forward(const void* z, const float* gamma, const float* beta, float* running_mean, float* running_var, int N,
                                          int L, int C, int C_param, float eps, float momentum, int act, float clamp_lo, float clamp_hi,
                                          long os_n, long os_t, void* y, float* mean, float* rstd, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    return bh_k_batchnorm_train_forward(z, gamma, beta, running_mean, running_var, N, L, C, C_param, eps, momentum, act, clamp_lo, clamp_hi,
                                        os_n, os_t, y, mean, rstd, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int bh_batchnorm_train_backward(const void* z, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                           const void* y, const void* dy, int N, int L, int C, int C_param, int act, float clamp_lo,
                                           float clamp_hi, long os_n, long os_t, void* dz, float* dgamma, float* dbeta, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    return bh_k_batchnorm_train_backward(z, gamma, beta, mean, rstd, y, dy, N, L, C, C_param, act, clamp_lo, clamp_hi, os_n, os_t, dz, dgamma,
                                         dbeta, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" size_t bh_dwconv1d_train_workspace(int N, int L, int C, int K, int pad) { return bh_k_dwconv_train_workspace(N, L, C, K, pad); }
extern "C" int bh_dwconv1d_train_backward(const void* x, const float* w, const void* dy, int N, int L, int C, int K, int pad, void* dx,
                                          float* dw, void* workspace, size_t workspace_bytes, void* stream) {
    return bh_k_dwconv_train_backward(x, w, dy, N, L, C, K, pad, dx, dw, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int bh_residual_act_train_forward(const void* a, const void* b, long M, int C, int act, unsigned int p_threshold, float inv_keep,
                                             unsigned long long seed, unsigned long long stream_id, void* y, void* stream) {
    return bh_k_residual_act_train_forward(a, b, M, C, act, p_threshold, inv_keep, seed, stream_id, y, (hipStream_t)stream);
}
extern "C" int bh_residual_act_train_backward(const void* a, const void* b, const void* dy, long M, int C, int act, unsigned int p_threshold,
                                              float inv_keep, unsigned long long seed, unsigned long long stream_id, void* da,
                                              void* stream) {
    return bh_k_residual_act_train_backward(a, b, dy, M, C, act, p_threshold, inv_keep, seed, stream_id, da, (hipStream_t)stream);
}
extern "C" size_t bh_ctc_head_train_workspace(long M, int F, int classes) { return bh_k_ctc_head_train_workspace(M, F, classes); }
extern "C" int bh_ctc_head_train_backward(const void* x, const float* w, const float* bias, const void* dlp, long M, int F, int classes,
                                          void* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    return bh_k_ctc_head_train_backward(x, w, bias, dlp, M, F, classes, dx, dw, db, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" size_t bh_sw_workspace(int n, int max_seq, int max_ref) { return bh_k_sw_workspace(n, max_seq, max_ref); }
extern "C" int bh_sw_align(const void* seqs, long seq_stride, const int32_t* seq_lengths, const void* refs, long ref_stride,
                           const int32_t* ref_lengths, int n, int match, int mismatch, int gap_open, int gap_extend, void* workspace,
                           size_t workspace_bytes, int32_t* result, uint32_t* ops, long ops_stride, int32_t* n_ops, void* stream) {
    return bh_k_sw_align(seqs, seq_stride, seq_lengths, refs, ref_stride, ref_lengths, n, match, mismatch, gap_open, gap_extend,
                         workspace, workspace_bytes, result, ops, ops_stride, n_ops, (hipStream_t)stream);
}
extern "C" int bh_sg_align(const void* seqs, long seq_stride, const int32_t* seq_lengths, const void* refs, long ref_stride,
                           const int32_t* ref_lengths, int n, int match, int mismatch, int gap_open, int gap_extend, void* workspace,
                           size_t workspace_bytes, int32_t* result, uint32_t* ops, long ops_stride, int32_t* n_ops, void* stream) {
    return bh_k_sg_align(seqs, seq_stride, seq_lengths, refs, ref_stride, ref_lengths, n, match, mismatch, gap_open, gap_extend,
                         workspace, workspace_bytes, result, ops, ops_stride, n_ops, (hipStream_t)stream);
}
extern "C" size_t bh_nw_workspace(int n, int max_seq, int max_ref, long max_band) {
    return bh_k_nw_workspace(n, max_seq, max_ref, max_band);
}
extern "C" int bh_nw_align(const void* seqs, long seq_stride, const int32_t* seq_lengths, const void* refs, long ref_stride,
                           const int32_t* ref_lengths, int n, int k, void* workspace, size_t workspace_bytes, int32_t* result,
                           uint32_t* ops, long ops_stride, int32_t* n_ops, void* stream) {
    return bh_k_nw_align(seqs, seq_stride, seq_lengths, refs, ref_stride, ref_lengths, n, k, workspace, workspace_bytes, result, ops,
                         ops_stride, n_ops, (hipStream_t)stream);
}
extern "C" int bh_map_sketch_tile(void) { return bh_k_map_sketch_tile(); }
extern "C" size_t bh_map_sketch_workspace(int n, long total_len) { return bh_k_map_sketch_workspace(n, total_len); }
extern "C" int bh_map_sketch(const void* codes, long stride, const int32_t* lengths, int n, int k, int w, void* workspace,
                             size_t workspace_bytes, int64_t* keys, int32_t* pos, int8_t* strand, long capacity, int32_t* offsets,
                             void* stream) {
    return bh_k_map_sketch(codes, stride, lengths, n, k, w, workspace, workspace_bytes, (long long*)keys, pos, strand, capacity, offsets,
                           (hipStream_t)stream);
}
extern "C" int bh_map_seed(const int64_t* qkeys, const int32_t* qpos, const int8_t* qstrand, const int32_t* q_offsets,
                           const int32_t* q_lengths, int n, long n_min, const int64_t* ukeys, const int32_t* ustart,
                           const int32_t* ucount, long n_ukeys, const int32_t* rpos, const int8_t* rstrand, int k, int max_occ,
                           int32_t* counts, const int64_t* offsets, int64_t* anchors, long capacity, void* stream) {
    return bh_k_map_seed((const long long*)qkeys, qpos, qstrand, q_offsets, q_lengths, n, n_min, (const long long*)ukeys, ustart, ucount,
                         n_ukeys, rpos, rstrand, k, max_occ, counts, (const long long*)offsets, (long long*)anchors, capacity,
                         (hipStream_t)stream);
}
extern "C" int bh_map_chain(const int64_t* anchors, const int32_t* contigs, const int32_t* offsets, int n, long n_anchors, int k,
                            int max_dist, int bandwidth, int32_t* f, int32_t* p, int32_t* chain, int32_t* result, void* stream) {
    return bh_k_map_chain((const long long*)anchors, contigs, offsets, n, n_anchors, k, max_dist, bandwidth, f, p, chain, result,
                          (hipStream_t)stream);
}
extern "C" int bh_map_extend_max(void) { return bh_k_map_extend_max(); }
extern "C" int bh_map_extend_band(void) { return bh_k_map_extend_band(); }
extern "C" int bh_map_extend(const int8_t* reads, long stride, const int32_t* read_len, int n_reads, const int8_t* ref, long ref_len,
                             const int32_t* ends, int n_ends, int32_t* result, uint32_t* runs, int runs_cap, void* stream) {
    return bh_k_map_extend(reads, stride, read_len, n_reads, ref, ref_len, ends, n_ends, result, runs, runs_cap, (hipStream_t)stream);
}
extern "C" int bh_signal_normalise(const int16_t* raw, const long* offsets, const float* cal_scale, const float* cal_offset, int n_reads,
                                   int strategy, double quantile_a, double quantile_b, double shift_mult, double scale_mult,
                                   double fixed_shift, double fixed_scale, int do_trim, double* shift, double* scale, int* weak,
                                   int* trim, void* stream) {
    return bh_k_signal_normalise(raw, offsets, cal_scale, cal_offset, n_reads, strategy, quantile_a, quantile_b, shift_mult,
                                 scale_mult, fixed_shift, fixed_scale, do_trim, shift, scale, weak, trim, (hipStream_t)stream);
}
extern "C" int bh_signal_chunks(const int16_t* raw, const long* offsets, const float* cal_scale, const float* cal_offset,
                                const double* shift, const double* scale, const int* weak, const int* chunk_read,
                                const long* chunk_start, const long* chunk_len, int n_chunks, int chunk_samples, void* out,
                                void* stream) {
    BH_REQUIRE(raw && offsets && cal_scale && cal_offset && shift && scale && weak && chunk_read && chunk_start && chunk_len && out,
               "signal_chunks: null pointer");
    return bh_k_signal_chunks(raw, offsets, cal_scale, cal_offset, shift, scale, weak, chunk_read, chunk_start, chunk_len,
                              n_chunks, chunk_samples, out, (hipStream_t)stream);
}
extern "C" int bh_set_option(const char* name, int value) {
    BH_REQUIRE(name != nullptr, "set_option: null name");
    const bh::OptionRow* row = bh::find_option(name);      // options.cpp: the one table of process-wide knobs
    BH_REQUIRE(row != nullptr, "set_option: unknown option '%s'", name);
    bh::g_opt.*row->member = row->normalise(value);
    return 0;
}
extern "C" size_t bh_crf_posterior_viterbi_workspace(int N, int T, int state_len) {
    return bh_k_posterior_viterbi_workspace(N, T, state_len);
}
extern "C" int bh_crf_posterior_viterbi(const void* scores, int N, int T, int state_len, float blank_score, void* workspace,
                                        int8_t* moves, int8_t* path, void* stream) {
    BH_REQUIRE(scores && workspace && moves && path, "crf_posterior_viterbi: null pointer");
    return bh_k_posterior_viterbi(scores, N, T, state_len, blank_score, workspace, moves, path, (hipStream_t)stream);
}
extern "C" size_t bh_crf_viterbi_workspace(int N, int T, int state_len) {
    size_t S = 1;
    for (int i = 0; i < state_len; ++i) S *= 4;
    return (size_t)N * T * S + 256;
}
extern "C" int bh_crf_viterbi(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score,
                              long stride_n, long stride_t, void* workspace, int8_t* moves, int8_t* path,
                              float* best, void* stream) {
    BH_REQUIRE(scores && workspace && moves && path, "crf_viterbi: null pointer");
    return bh_k_crf_viterbi(scores, N, T, state_len, layout_5s, blank_score, stride_n, stride_t, workspace, nullptr,
                            moves, path, best, (hipStream_t)stream);
}
