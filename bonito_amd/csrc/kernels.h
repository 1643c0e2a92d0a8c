// Internal launcher prototypes (one per HIP translation unit). The public C ABI in
// include/bonito_hip.h is a thin shell over these (bonito_amd/csrc/abi.cpp for the operators,
// engine.cpp for the encoder).
// All pointers are device pointers; all launchers are asynchronous on `stream` and return
// 0 on success (error text via bh_last_error()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bonito_hip.h"      // enum bh_lstm_family

// gemm.hip
int bh_k_linear(const void* X, const void* W, const float* bias, void* out, int M, int N, int K,
                int ldx, int ldw, int ldo, int act, float scale, float clamp_lo, float clamp_hi,
                int gated, int row_div, long row_s_hi, long row_s_lo, int row_lim, hipStream_t stream,
                const void* residual = nullptr, int ldres = 0, float res_scale = 1.0f);
int bh_k_linear_last_kernel();     // test hook: the kernel the last launch took (1 = v1, 2 = v2, 3 = v3, 5 / 6 = v5 on 32x32x16 / 16x16x32); not thread-safe

// conv.hip
int bh_k_conv_first(const void* signal, const float* w, const float* bias, void* out, int N, int Lin,
                    int Lout, int Cout, int K, int stride, int pad, int act, float clamp_lo,
                    float clamp_hi, long os_n, long os_t, hipStream_t stream);
int bh_k_conv_igemm(const void* in, const void* wpk, const float* bias, void* out, int N, int Lin,
                    int Lout, int Cin, int Cout, int K, int stride, int pad, int act, float clamp_lo,
                    float clamp_hi, long os_n, long os_t, hipStream_t stream);
// test hook: the kernel and instance the last convolution launch took, as a bh_conv_kernel code (include/bonito_hip.h); every launcher
// of conv.hip and bh_k_dwconv note theirs. A host-side static: process-wide, not thread-safe
int bh_k_conv_last_kernel();
void bh_k_conv_note_kernel(int code);

// lstm.hip
// Launch geometry of a recurrent kernel family: the ONE statement of how many workgroups a launch of n rings takes and, inverted,
// how many rings fit one launch. The workgroups of a launch spin on each other, so all of them must be resident at once; rings are
// dealt to the 8 XCDs, hence the groups of 8. The launcher's grid and co-residency guard and every caller that splits a batch
// (bh_k_lstm_run_layer) read it from here.
// (enum bh_lstm_family: include/bonito_hip.h)
struct bh_lstm_geometry {
    int ring_chunks = 16;        // chunks per ring
    int wgs_per_group = 0;       // workgroups that serve 8 workgroup slots, one per XCD (0: the kernel does not cover H)
    int rings_per_slot = 1;      // rings a workgroup slot carries
    int wgs_per_cu = 1;          // workgroups resident on one CU
    bool unlimited = false;      // one workgroup per ring and no spin across workgroups: any number of rings per launch
    int grid(int n_rings) const {
        if (unlimited) return n_rings;
        const int per_group = 8 * rings_per_slot;
        return 8 * ((n_rings + per_group - 1) / per_group) * wgs_per_group;
    }
    int resident(int cus) const { return cus * wgs_per_cu; }       // workgroups the device holds at once
    int rings_per_launch(int cus) const {                          // 0: the device is too small for one group of rings
        if (unlimited) return INT32_MAX;
        return wgs_per_group > 0 ? resident(cus) / (8 * wgs_per_group) * 8 * rings_per_slot : 0;
    }
};
// How a recurrent kernel wants a weight matrix laid out (lstm_pack.h packs them).
enum bh_lstm_layout {
    BH_LSTM_W_ROWS = 0,        // fp16 rows in torch order: the operand of the gate GEMM
    BH_LSTM_W_FRAGS,           // per-wave MFMA fragments of 16 units (bh_lstm_pack_whh)
    BH_LSTM_W_TILES,           // tiles of 4 * MT units per slice (MT: the instance's)
    BH_LSTM_W_WIDE_ROWS,       // fp16 rows, and the bias, in the wide kernel's gate order: the operand of ITS gate GEMM
    BH_LSTM_W_LAYOUTS
};
constexpr int BH_LSTM_WIDE_MT = 2;      // the wide kernel's tiles: 8 units
// Variants of an instance (bh_k_lstm_find). BH_LSTM_V_OUTPUT is bit 1 of bh_lstm_layer_family's and bh_lstm_launch_plan's flags.
enum { BH_LSTM_V_OUTPUT = 2,            // hand-off through the output tensor where the family's default is the ring buffer (wide: RX = false)
       BH_LSTM_V_STATS = 4 };           // the instance with section stamps, taken under "lstm_tune" bit 2 where it exists
// One row of the instance table of lstm.hip: a (family, H, variant) that is compiled, with what the kernel was compiled with and what
// a launch of it needs. The ONE statement of which widths a family serves; every caller reads it from here.
struct bh_lstm_instance {
    bh_lstm_family family;
    int H, variant;
    int nks, mt, key_flags;     // template key: H / 32, M tiles per wave (0: none), bit 0 = the kernel's STREAM / RX parameter, bit 1 = STATS
    const void* kernel;
    const char* name;           // as bh_encoder_describe prints it
    int args;                   // which argument struct the kernel takes (lstm.hip)
    int block;
    int lds_bytes;              // dynamic LDS
    bool raise_lds;             // the max-dynamic-LDS attribute must be raised first
    bh_lstm_geometry geo;
    int slots_per_ring;         // XCD agreement slots (0: no agreement)
    size_t ex_bytes;            // exchange ring buffer: bytes per ring and time slot (the buffer is [4][R] of them), 0: none
    bool projects;              // the input projection is inside: reads x [T][N][H] (in_size == H), W_ih and the bias go to the kernel.
                                // false: reads the gate pre-activations [T][N][4H] of a GEMM with W_ih and the bias
    bh_lstm_layout w_ih, w_hh;
};
const bh_lstm_instance* bh_k_lstm_find(int family, int H, int variant);      // null: no such instance
inline bool bh_k_lstm_serves(int family, int H) { return bh_k_lstm_find(family, H, 0) != nullptr; }
// One launch of an fp16 recurrent kernel. The tensors keep the row stride of the whole batch (N chunks = R rings); a launch runs
// n_rings of them from the pointers it is given.
struct bh_lstm_launch {
    bh_lstm_family family;
    const void* input;          // x or the gate pre-activations (bh_lstm_instance::projects)
    const void* w_ih;           // in the instance's layouts; w_ih and bias are read by the projecting kernels only
    const void* w_hh;
    const float* bias;
    void* h_out;
    void* ex;                   // exchange ring buffer, or null: hand-off through the output tensor (which the caller has filled with 0xFFFF)
    int T, N, H;
    int R, n_rings;             // ring stride of `ex` = rings of the whole batch; rings of this launch
    int reverse;
    int* err_flag;
    int* xcc_ws;                // bh_k_lstm_ws_bytes
    int write_through;          // "lstm_force_slow"
    int tune;                   // "lstm_tune"
    int arm;                    // fill `ex` with the sentinel first: once per layer
};
// The only function that launches an fp16 recurrent kernel.
int bh_k_lstm_launch(const bh_lstm_launch& l, hipStream_t stream);
// All rings of a layer (layer.n_rings == layer.R, pointers at ring 0), at most rings_per_launch per launch; `pair`: BH_LSTM_WGX serves
// more rings than that two per workgroup (BH_LSTM_WGX2, twice as many per launch) instead of in two launches.
int bh_k_lstm_run_layer(const bh_lstm_launch& layer, int rings_per_launch, bool pair, hipStream_t stream);
// test hook: the launch bh_k_lstm_launch (BH_LSTM_Q8: bh_k_lstm_layer_q8) would make of n_rings = R rings with `arm` set on a device of
// `cus` CUs, as BH_LSTM_PLAN_RECORD integers (include/bonito_hip.h lists them); no device call
int bh_k_lstm_launch_plan(int family, int H, int flags, int n_rings, int cus, int32_t* out, int n_out);
size_t bh_k_lstm_ws_bytes(int N, int H);
int bh_k_fill_u16(void* dst, uint16_t value, size_t count, hipStream_t stream);

// crf.hip
int bh_k_crf_viterbi(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score,
                     long s_n, long s_t, void* bp_ws, float* alpha_ws, int8_t* moves, int8_t* path,
                     float* best_score, hipStream_t stream);

int bh_k_crf_revcomp(const void* in, void* out, int N, int T, int state_len, int layout_5s, long s_n, long s_t,
                     hipStream_t stream);

// seqdist.hip (mode 0: Log scan, 1: Max scan + traceback, 2: Log scan with a free start)
size_t bh_k_crf_seq_workspace(int N, int T, int Lmax, int state_len);
int bh_k_crf_seq(const void* scores, int N, int T, int state_len, int layout_5s, float blank, long s_n, long s_t,
                 const void* targets, int target_bytes, int Lmax, const int* lens, void* workspace, float* out, int* align,
                 int mode, hipStream_t stream);
int bh_k_crf_logz_dense(const void* scores, int N, int T, int state_len, int layout_5s, float blank, long s_n, long s_t,
                        float* out, hipStream_t stream);

// seqdist_grad.hip (alpha-beta passes: logz and its gradient, the posterior occupancy of every edge, from one launch)
size_t bh_k_crf_seq_grad_workspace(int N, int T, int Lmax, int state_len);
int bh_k_crf_seq_grad(const void* scores, int N, int T, int state_len, int layout_5s, float blank, long s_n, long s_t,
                      const void* targets, int target_bytes, int Lmax, const int* lens, const float* weight, void* workspace,
                      float* out, void* grad, long g_n, long g_t, int grad_fp32, int accumulate, hipStream_t stream);
size_t bh_k_crf_logz_dense_grad_workspace(int N, int T, int state_len);
int bh_k_crf_logz_dense_grad(const void* scores, int N, int T, int state_len, int layout_5s, float blank, long s_n, long s_t,
                             const float* weight, void* workspace, float* out, void* grad, long g_n, long g_t, int grad_fp32,
                             hipStream_t stream);

// ctc_loss.hip (the CTC loss of bonito.ctc: nll, the label-smoothing numerator and - with_grad - the gradient, from one launch)
size_t bh_k_ctc_loss_workspace(int N, int T, int C, int Lmax, int grad);
int bh_k_ctc_loss(const void* log_probs, int logp_fp32, int N, int T, int C, long s_t, long s_n, const void* targets, int target_bytes,
                  int Lmax, const int* lens, const float* smooth_w, const float* weight, const float* smooth_weight, void* workspace,
                  float* nll, float* smooth, void* grad, long g_t, long g_n, int grad_fp32, int accumulate, int with_grad,
                  hipStream_t stream);
int bh_k_ctc_loss_last_kernel();   // test hook: the bh_ctc_loss_kernel code of the instance that served the last call; not thread-safe

// lstm_train.hip (one LSTM layer for training: the forward that keeps the gates and c, and the backward; every pointer a device pointer)
size_t bh_k_lstm_train_saved_bytes(int T, int N, int H);
size_t bh_k_lstm_train_backward_workspace(int T, int N, int H);
int bh_k_lstm_train_workgroups(int N);       // workgroups of the two recurrent kernels: one per tile of 16 chunks
int bh_k_lstm_train_forward(const void* x, const float* w_ih, const float* w_hh, const float* bias, int T, int N, int H, int reverse,
                            void* h_out, void* saved, size_t saved_bytes, hipStream_t stream);
int bh_k_lstm_train_backward(const void* x, const float* w_ih, const float* w_hh, const void* h, const void* saved, const void* dh, int T,
                             int N, int H, int reverse, void* dx, float* dw_ih, float* dw_hh, float* dbias, void* workspace,
                             size_t workspace_bytes, hipStream_t stream);

// train_layers.hip (the convolution and the linear / CRF-head layer for training: forward on the rounded master weights, and the backward)
size_t bh_k_conv_train_workspace(int N, int Lin, int Cin, int Cout, int K, int stride, int pad);
int bh_k_conv_train_forward(const void* x, const float* w, const float* bias, int N, int Lin, int Cin, int Cout, int K, int stride, int pad,
                            int act, float clamp_lo, float clamp_hi, long os_n, long os_t, void* y, void* workspace, size_t workspace_bytes,
                            hipStream_t stream);
int bh_k_conv_train_backward(const void* x, const float* w, const float* bias, const void* y, const void* dy, int N, int Lin, int Cin, int Cout,
                             int K, int stride, int pad, int act, float clamp_lo, float clamp_hi, long os_n, long os_t, void* dx, float* dw,
                             float* db, void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t bh_k_linear_train_workspace(int T, int N, int K, int C);
int bh_k_linear_train_forward(const void* x, const float* w, const float* bias, int T, int N, int K, int C, int act, float scale,
                              float clamp_lo, float clamp_hi, int batch_major, void* y, void* workspace, size_t workspace_bytes,
                              hipStream_t stream);
int bh_k_linear_train_backward(const void* x, const float* w, const void* y, const void* dy, int T, int N, int K, int C, int act, float scale,
                               float clamp_lo, float clamp_hi, int batch_major, void* dx, float* dw, float* db, void* workspace,
                               size_t workspace_bytes, hipStream_t stream);

// transformer_train.hip (what a transformer encoder layer adds to training: the backward of bh_k_rmsnorm_residual, and fc1 + SwiGLU)
size_t bh_k_batchnorm_train_workspace(int N, int L, int C);
int bh_k_batchnorm_train_forward(const void* z, const float* gamma, const float* beta, float* running_mean, float* running_var, int N, int L,
                                 int C, int C_param, float eps, float momentum, int act, float clamp_lo, float clamp_hi, long os_n, long os_t,
                                 void* y, float* mean, float* rstd, void* workspace, size_t workspace_bytes, hipStream_t stream);
int bh_k_batchnorm_train_backward(const void* z, const float* gamma, const float* beta, const float* mean, const float* rstd, const void* y,
                                  const void* dy, int N, int L, int C, int C_param, int act, float clamp_lo, float clamp_hi, long os_n, long os_t,
                                  void* dz, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t bh_k_rmsnorm_train_workspace(long M, int D);
int bh_k_rmsnorm_train_backward(const void* a, const void* x, const float* w, const void* dy, long M, int D, float alpha, float eps, void* da,
                                void* dx, float* dw, void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t bh_k_gated_linear_train_workspace(long M, int D, int F);
int bh_k_gated_linear_train_forward(const void* x, const float* w, long M, int D, int F, void* h, void* workspace, size_t workspace_bytes,
                                    hipStream_t stream);
int bh_k_gated_linear_train_backward(const void* x, const float* w, const void* dh, long M, int D, int F, void* dx, float* dw, void* workspace,
                                     size_t workspace_bytes, hipStream_t stream);

// quartznet_train.hip (what training a bonito.ctc model adds: the depthwise backward, residual + activation + dropout, the head backward)
size_t bh_k_dwconv_train_workspace(int N, int L, int C, int K, int pad);
int bh_k_dwconv_train_backward(const void* x, const float* w, const void* dy, int N, int L, int C, int K, int pad, void* dx, float* dw,
                               void* workspace, size_t workspace_bytes, hipStream_t stream);
int bh_k_residual_act_train_forward(const void* a, const void* b, long M, int C, int act, unsigned int p_threshold, float inv_keep,
                                    unsigned long long seed, unsigned long long stream_id, void* y, hipStream_t stream);
int bh_k_residual_act_train_backward(const void* a, const void* b, const void* dy, long M, int C, int act, unsigned int p_threshold,
                                     float inv_keep, unsigned long long seed, unsigned long long stream_id, void* da, hipStream_t stream);
size_t bh_k_ctc_head_train_workspace(long M, int F, int classes);
int bh_k_ctc_head_train_backward(const void* x, const float* w, const float* bias, const void* dlp, long M, int F, int classes, void* dx,
                                 float* dw, float* db, void* workspace, size_t workspace_bytes, hipStream_t stream);

// align.hip (Smith-Waterman, affine gaps, traceback; the lengths are host arrays)
size_t bh_k_sw_workspace(int n, int max_seq, int max_ref);
int bh_k_sw_align(const void* seqs, long seq_stride, const int* seq_lens, const void* refs, long ref_stride, const int* ref_lens,
                  int n, int match, int mismatch, int gap_open, int gap_extend, void* workspace, size_t workspace_bytes,
                  int* result, unsigned* ops, long ops_stride, int* n_ops, hipStream_t stream);
// the semi-global mode of the same kernels (free end gaps on both sequences, the CIGAR covers both completely); bh_k_sw_workspace
int bh_k_sg_align(const void* seqs, long seq_stride, const int* seq_lens, const void* refs, long ref_stride, const int* ref_lens,
                  int n, int match, int mismatch, int gap_open, int gap_extend, void* workspace, size_t workspace_bytes,
                  int* result, unsigned* ops, long ops_stride, int* n_ops, hipStream_t stream);

// mapper.hip (the read mapper: minimizer sketch, seeding against a sorted index, chaining; the sketch's lengths are a host array)
int bh_k_map_sketch_tile();
size_t bh_k_map_sketch_workspace(int n, long total_len);
int bh_k_map_sketch(const void* codes, long stride, const int* lengths, int n, int k, int w, void* workspace, size_t workspace_bytes,
                    long long* keys, int* pos, int8_t* strand, long capacity, int* offsets, hipStream_t stream);
int bh_k_map_seed(const long long* qkeys, const int* qpos, const int8_t* qstrand, const int* q_offsets, const int* q_lengths, int n,
                  long n_min, const long long* ukeys, const int* ustart, const int* ucount, long n_ukeys, const int* rpos,
                  const int8_t* rstrand, int k, int max_occ, int* counts, const long long* offsets, long long* anchors, long capacity,
                  hipStream_t stream);
int bh_k_map_chain(const long long* anchors, const int* contigs, const int* offsets, int n, long n_anchors, int k, int max_dist,
                   int bandwidth, int* f, int* p, int* chain, int* result, hipStream_t stream);
// end extension of the mappings (one wave per end; every array is a device array, an end that does not fit is flagged, not read)
int bh_k_map_extend_max();
int bh_k_map_extend_band();
int bh_k_map_extend(const int8_t* reads, long stride, const int* read_len, int n_reads, const int8_t* ref, long ref_len, const int* ends,
                    int n_ends, int* result, unsigned* runs, int runs_cap, hipStream_t stream);

// nw.hip (banded global alignment under unit costs with a traceback; one band half-width k per call; the lengths are host arrays)
size_t bh_k_nw_workspace(int n, int max_seq, int max_ref, long max_band);
int bh_k_nw_align(const void* seqs, long seq_stride, const int* seq_lens, const void* refs, long ref_stride, const int* ref_lens,
                  int n, int k, void* workspace, size_t workspace_bytes, int* result, unsigned* ops, long ops_stride, int* n_ops,
                  hipStream_t stream);

// beam.hip: the decode stage on koi-layout scores. The three calls share ONE workspace layout (decode_workspace); a beam search's
// launches - backward scan, forward / posterior scan (fused into the beam kernel or not, on the helper stream or not), beam kernel
// instance, selection - are decided by ONE pure function of shape, options and CU count (beam_plan), which the entry point executes.
size_t bh_k_beam_workspace(int N, int T, int state_len);                    // bh_k_beam_search and bh_k_crf_logz
size_t bh_k_posterior_viterbi_workspace(int N, int T, int state_len);       // the same regions + the posterior back-pointer plane
int bh_k_posterior_viterbi(const void* scores, int N, int T, int state_len, float blank, void* workspace, int8_t* moves,
                           int8_t* path, hipStream_t stream);
// test hook: beam_plan and the layout for this shape under the current options, as BH_BEAM_PLAN_RECORD integers (include/bonito_hip.h lists them); no device call
int bh_k_beam_search_plan(int N, int T, int state_len, int cu_count, int debug, int32_t* out, int n_out);
int bh_k_crf_logz(const void* scores, int N, int T, int state_len, float blank, void* workspace, double* logz_out,
                   hipStream_t stream);
int bh_k_beam_search(const void* scores, int N, int T, int state_len, int beam_width, float beam_cut,
                     float blank, float q_scale, float q_offset, void* workspace, int8_t* sequence,
                     int8_t* qstring, int8_t* moves, float* qfloat, hipStream_t stream);

// attention.hip
int bh_k_attention(const void* qkv, void* out, const float* cos_sin, int N, int T, int nhead, int head_dim,
                   int win_left, int win_right, hipStream_t stream);
int bh_k_rmsnorm_residual(const void* a, const void* x, const float* w, void* out, long M, int D, float alpha,
                          float eps, hipStream_t stream);
// The block-per-workgroup kernel behind bh_k_attention, behind its checks (attn_block.h: attn_block_check). lse == nullptr: inference;
// otherwise the training forward (attention_train.hip), which also writes lse = m + ln(sum) of every query's softmax row, fp32 [N][nhead][T]
int bh_k_attention_block(const void* qkv, void* out, const float* cos_sin, int N, int T, int nhead, int win_left, int win_right, float* lse,
                         hipStream_t stream);
// The windows the block kernels serve: the key tiles (of 16) one wave of 16 queries can see must number at most those of the widest instance
constexpr int BH_ATTN_MAX_TILES = 26;
inline long bh_k_attention_tiles(int win_left, int win_right) { return (16 + (long)win_left + win_right + 15) / 16; }
inline bool bh_k_attention_serves(int win_left, int win_right) {
    return win_left >= 0 && win_right >= 0 && bh_k_attention_tiles(win_left, win_right) <= BH_ATTN_MAX_TILES;
}

// attention_train.hip (rotary + sliding-window attention for training: the forward that keeps lse, and the backward; device pointers)
size_t bh_k_attention_train_saved_bytes(int N, int T, int nhead);
size_t bh_k_attention_train_backward_workspace(int N, int T, int nhead, int win_left, int win_right);
int bh_k_attention_train_forward(const void* qkv, const float* cos_sin, int N, int T, int nhead, int head_dim, int win_left, int win_right,
                                 void* out, void* saved, size_t saved_bytes, hipStream_t stream);
int bh_k_attention_train_backward(const void* qkv, const float* cos_sin, const void* out, const void* saved, const void* dout, int N, int T,
                                  int nhead, int head_dim, int win_left, int win_right, void* dqkv, void* workspace, size_t workspace_bytes,
                                  hipStream_t stream);

// ctc.hip
int bh_k_dwconv(const void* in, const float* w, void* out, int N, int Lin, int Lout, int C, int K, int stride,
                int pad, hipStream_t stream);
int bh_k_ctc_head(const void* in, const float* w, const float* bias, void* out, long M, int features, int classes,
                  hipStream_t stream);
int bh_k_ctc_greedy(const float* logp, const long* offs, int R, int C, float qscale, float qbias, int8_t* seq,
                    int8_t* qual, int* path, int* count, hipStream_t stream);
size_t bh_k_ctc_beam_workspace(long total_steps, int R, int C, int beam_size);
int bh_k_ctc_prefix_beam(const float* logp, const long* offs, int R, int C, int beam_size, float threshold, void* workspace,
                         int8_t* labels, int* path, int* count, hipStream_t stream);
// conv1 -> conv2 -> conv3 of an LSTM model's front end in one kernel (conv_front3_kernel). _shape_ok: do the launcher's own arguments have
// an instance (pure; the launcher requires it)? _option_ok: do "conv_fuse" / "conv_ws" allow it? _ok: the engine's question - the layers'
// channel counts and strides, and both of the former
int bh_k_conv_front3_shape_ok(int K1, int K2, int c3_out, int K3, int s3);
int bh_k_conv_front3_option_ok(int c3_out);
int bh_k_conv_front3_ok(int c1_eff, int K1, int s1, int c2_in_eff, int c2_eff, int K2, int s2, int c3_in_eff, int c3_out, int K3, int s3);
int bh_k_conv_front3(const void* signal, int N, int L0, const float* w1, const float* b1, int K1, int pad1, int act1, float lo1, float hi1,
                     const void* w2pk, const float* b2, int K2, int pad2, int act2, float lo2, float hi2, const void* w3pk,
                     const float* b3, int Cout3, int K3, int stride3, int pad3, int act3, float lo3, float hi3, void* out, long os_n,
                     long os_t, hipStream_t stream);
int bh_k_linear_qkv_rotary(const void* X, const void* W, const float* bias, void* out, int M, int D, int K, const float* cos_sin,
                           int T, float qscale, hipStream_t stream);
int bh_k_attention_prerotated(const void* qkv, void* out, int N, int T, int nhead, int head_dim, int win_left, int win_right,
                              hipStream_t stream);
// The windows the ring kernels serve - the ONE statement of it: the launcher's guard and the engine's dispatch both call this. A wave's 18
// key tiles start 128 keys left of its first query and end 159 keys right of it, and its last query is the first + 15: 128 to the left,
// 159 - 15 = 144 to the right (the staged rows of a block end at its last query + 144 as well). Everything else is bh_k_attention's.
inline bool bh_k_attention_ring_serves(int win_left, int win_right) {
    return win_left >= 0 && win_right >= 0 && win_left <= 128 && win_right <= 144;
}
// signal.hip
int bh_k_signal_normalise(const int16_t* raw, const long* offs, const float* cal_scale, const float* cal_offset, int R,
                          int strategy, double qa, double qb, double shift_mult, double scale_mult, double fixed_shift,
                          double fixed_scale, int do_trim, double* shift, double* scale, int* weak, int* trim, hipStream_t stream);
int bh_k_signal_chunks(const int16_t* raw, const long* offs, const float* cal_scale, const float* cal_offset, const double* shift,
                       const double* scale, const int* weak, const int* chunk_read, const long* chunk_start, const long* chunk_len,
                       int n_chunks, int L, void* out, hipStream_t stream);

// lstm_q8.hip: 8-bit recurrent path Q8-1
int bh_k_lstm_q8_units(int H, int variant);
bh_lstm_geometry bh_k_lstm_q8_geometry(int H, int variant);
size_t bh_k_lstm_q8_tile_bytes(int H);
int bh_k_lstm_q8_pack(const float* w, int H, int U, int8_t* packed, float* scale);
int bh_k_quantise_rows(const void* x, void* out, int T, int N, int H, int R, float bound, hipStream_t stream);
int bh_k_lstm_q8_arm(void* ex, int R, int H, hipStream_t stream);
int bh_k_lstm_layer_q8(const void* xq, const void* wih, const void* whh, const float* sx, const float* sh, const float* bias,
                       void* hq_out, void* h16_out, void* ex, int T, int N, int H, int R, int n_rings, int reverse, int* err_flag,
                       hipStream_t stream, int* xcc_ws, int flags, int variant, int* dbg, unsigned max_spins);
int bh_k_lstm_q8_launch_plan(int H, int variant, int n_rings, int cus, int32_t* out);      // bh_k_lstm_launch_plan for BH_LSTM_Q8
