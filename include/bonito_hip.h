/* bonito_hip.h -- C ABI of libbonito_hip.so, the MI355X (gfx950) engine for bonito's
 * chunked-signal inference hot path:  signal chunks -> encoder -> CRF scores -> decode.
 *
 * This is the drop-in boundary.  Each entry point replaces one FFI/library call the reference makes
 * on this path (paths relative to /root/reference):
 *
 *   bh_encoder_create / bh_encoder_forward
 *        koi.lstm.update_graph(encoder, batchsize, chunksize, quantize)        bonito/crf/model.py:240-246
 *        + SeqdistModel.forward -> self.encoder(x) (cuDNN/cuBLAS/flash-attn)   bonito/crf/model.py:193-194
 *        + transformer use_koi (NTC, expand_blanks=False output)               bonito/transformer/model.py:136-146
 *        + bonito.ctc Model.forward (QuartzNet + log_softmax)                  bonito/ctc/model.py:35-37,195-207
 *   bh_beam_search
 *        koi.decode.beam_search(scores, beam_width, beam_cut, scale, offset, blank_score)
 *                                                                              bonito/crf/basecall.py:36-40
 *   bh_crf_viterbi / bh_crf_logz / bh_crf_posterior_viterbi
 *        koi.ctc.{logZ_cu_sparse, fwd_scores_cu_sparse, bwd_scores_cu_sparse}, SequenceDist.posteriors
 *        behind CTC_CRF.logZ / viterbi / decode_batch                          bonito/crf/model.py:47-67,98-103,196-199
 *   bh_crf_seq_logz / bh_crf_seq_viterbi (+ bh_crf_seq_logz_free, bh_crf_logz_dense)
 *        koi.ctc.{logZ_cu, viterbi_alignments} behind CTC_CRF.ctc_loss / ctc_viterbi_alignments, SeqdistModel.loss
 *                                                                              bonito/crf/model.py:126-143,204-207
 *   bh_crf_seq_logz_grad / bh_crf_logz_dense_grad
 *        the backward of koi.ctc.{logZ_cu, logZ_cu_sparse} (autograd of CTC_CRF.ctc_loss) and SequenceDist.posteriors
 *                                                                              bonito/crf/model.py:47-67,126-139
 *   bh_ctc_loss / bh_ctc_loss_grad
 *        torch.nn.functional.ctc_loss (and its backward) behind Model.ctc_label_smoothing_loss / Model.loss
 *                                                                              bonito/ctc/model.py:48-57
 *   bh_lstm_train_forward / bh_lstm_train_backward
 *        torch.nn.LSTM under autocast, and its autograd, as the reference's LSTM layer wraps it   bonito/nn.py:353-397
 *   bh_attention_train_forward / bh_attention_train_backward
 *        RotaryEmbedding + flash_attn_qkvpacked_func(qkv, window_size=) and their autograd          bonito/transformer/model.py:58-75
 *   bh_rmsnorm_train_backward / bh_gated_linear_train_forward / bh_gated_linear_train_backward
 *        the autograd of RMSNorm(attn / ff + deepnorm_alpha * x) and of GatedMlp's fc1 + SwiGLU         bonito/transformer/model.py:83-133
 *   bh_batchnorm_train_forward / bh_batchnorm_train_backward
 *        torch.nn.BatchNorm1d in training mode behind a Convolution (activation(norm(conv(x)))) and its autograd   bonito/nn.py:222-241
 *   bh_dwconv1d_train_backward / bh_residual_act_train_forward / bh_residual_act_train_backward / bh_ctc_head_train_backward
 *        the autograd of a QuartzNet Block and Decoder: Conv1d(groups=C), the residual add with activation and Dropout, and
 *        log_softmax(Conv1d(kernel_size=1))                                     bonito/ctc/model.py:90-207
 *   bh_sw_align
 *        parasail.sw_trace_striped_32(seq, ref, 8, 4, parasail.dnafull) behind evaluate's align() and util.accuracy
 *                                                                              bonito/cli/evaluate.py:37-67, bonito/util.py:346-368
 *   bh_nw_align / bh_sg_align
 *        edlib.align(query, ref, task="path") and parasail.sg_trace_scan_32(query, ref, 10, 2, dnafull) behind the basespace
 *        duplex caller                                                         bonito/cli/duplex.py:224-300
 *   bh_map_sketch / bh_map_seed / bh_map_chain / bh_map_extend
 *        mappy.Aligner(reference).map(sequence) behind `bonito basecaller --reference`, as far as seeding and chaining go; defined by
 *        tests/mapper_ref.py, minimap2 parity is not claimed                   bonito/aligner.py:1-63
 *   bh_ctc_greedy_decode / bh_ctc_beam_search
 *        fast_ctc_decode.viterbi_search / beam_search                          bonito/ctc/model.py:39-46
 *   bh_linear, bh_conv1d_*, bh_lstm_layer, ...  (operator level, used by the parity tests)
 *        torch.nn.Linear / Conv1d / LSTM kernels behind bonito/nn.py:27-38,222-241,396-415
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.  Device pointers are raw HIP device addresses.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All launches are asynchronous;
 *     nothing here synchronises the device unless documented.
 *   - every function returns 0 on success, non-zero on error; bh_last_error() returns a
 *     thread-local message.  Nothing ever falls back to a CPU path.
 *   - caller owns input/output buffers; engines own their weights (copied at create) and workspace.
 *   - an engine handle is not re-entrant: one handle per GPU worker thread (the reference drives
 *     compute_scores from a single ThreadIterator, bonito/multiprocessing.py:20-24).
 */
#ifndef BONITO_HIP_H
#define BONITO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BH_ABI_VERSION 1

/* activations (bonito.nn `layers` registry names: swish, tanh, relu; nn.py:22-23,54-56) */
enum { BH_ACT_NONE = 0, BH_ACT_SWISH = 1, BH_ACT_TANH = 2, BH_ACT_RELU = 3 };

/* layer kinds understood by bh_encoder_create (bonito.nn registry names in comments) */
enum {
    BH_LAYER_CONV = 1,        /* convolution  (nn.py:222; BatchNorm folded by the caller as nn.py:447-454) */
    BH_LAYER_LSTM = 2,        /* lstm         (nn.py:396) */
    BH_LAYER_LINEAR_CRF = 3,  /* linearcrfencoder (nn.py:269) */
    BH_LAYER_CLAMP = 4,       /* clamp        (nn.py:60) -- fused into the producing kernel */
    BH_LAYER_TRANSFORMER = 5, /* transformerencoderlayer (transformer/model.py:83) */
    BH_LAYER_UPSAMPLE = 6,    /* linearupsample (nn.py:140) */
    BH_LAYER_TCS_BLOCK = 7,   /* reserved */
    BH_LAYER_CTC_DECODER = 8, /* bonito.ctc Decoder: 1x1 conv + log_softmax (ctc/model.py:195-207); final layer */
    BH_LAYER_DWCONV = 9,      /* depthwise half of TCSConv1d (ctc/model.py:99-103): groups = channels, no bias */
    BH_LAYER_RESIDUAL_PROJ = 10, /* Block.residual (ctc/model.py:166-167): 1x1 conv + folded BN of the block input,
                                  * kept aside and added by the next BH_LAYER_CONV whose `add_residual` is set */
    BH_LAYER_LINEAR = 11      /* linear (nn.py:27-52): y = x W^T + b on the feature axis, any layout
                               * (dna_r10.4.1@v4.0.toml:101-104: 1024 -> 256 between the LSTM stack and the CRF head) */
};

/* One layer of an encoder.  All weight pointers are HOST fp32 arrays in torch's native layout; the
 * engine packs / rounds them to fp16 once at create time.  Unused fields are 0 / NULL. */
typedef struct bh_layer {
    int32_t kind;
    int32_t in_size;     /* conv: in channels; lstm/linear: in features; transformer: d_model */
    int32_t out_size;    /* conv: out channels; lstm: hidden; linear_crf: n_base^(state_len+1) (+ blanks if no blank_score) */
    int32_t winlen, stride, padding;   /* conv */
    int32_t activation;  /* BH_ACT_* */
    int32_t reverse;     /* lstm */
    int32_t nhead, dim_ff, win_left, win_right;   /* transformer */
    int32_t scale_factor;               /* upsample */
    int32_t groups;      /* conv: 1 */
    int32_t add_residual;               /* conv (pointwise): add the pending residual projection before the activation */
    int32_t quantize;    /* lstm: 1 = 8-bit recurrent path Q8-1 where the kernel covers the shape (koi's `quantize`, crf/model.py:245);
                            hidden sizes 144 and 336 have an 8-bit kernel and no fp16 one: such a layer is accepted only with quantize = 1 */
    int32_t reserved_i[1];
    float scale;         /* linear_crf: multiply after activation (0 = none) */
    float clamp_lo, clamp_hi;           /* clamp */
    float blank_score;   /* linear_crf with fixed blank (scores keep the 4S koi layout) */
    float alpha;         /* transformer: deepnorm_alpha */
    float eps;           /* transformer: rmsnorm eps */
    float reserved_f[2];
    const float* w0;     /* conv [Cout][Cin/groups][K]; lstm W_ih [4H][I]; linear [out][in]; transformer Wqkv [3D][D] */
    const float* b0;     /* conv bias [Cout]; lstm b_ih [4H]; linear bias; transformer: NULL */
    const float* w1;     /* lstm W_hh [4H][H]; transformer out_proj.weight [D][D] */
    const float* b1;     /* lstm b_hh [4H]; transformer out_proj.bias [D] */
    const float* w2;     /* transformer ff.fc1.weight [2F][D] */
    const float* w3;     /* transformer ff.fc2.weight [D][F] */
    const float* w4;     /* transformer norm1.weight [D] */
    const float* w5;     /* transformer norm2.weight [D] */
} bh_layer_t;

typedef struct bh_encoder bh_encoder_t;

const char* bh_last_error(void);
int bh_abi_version(void);
/* sizeof(bh_layer_t) as compiled into the library (bindings check their struct mirror against it) */
size_t bh_sizeof_layer(void);
/* number of visible HIP devices, or <0 on error */
int bh_device_count(void);

/* ---- encoder engine -------------------------------------------------------------------------- */
/* Build an engine for a linear chain of layers on HIP device `device`.  Workspace is sized for
 * batches of up to max_batch chunks of up to max_chunk samples (batch is padded to 16 internally). */
int bh_encoder_create(const bh_layer_t* layers, int n_layers, int device, int max_batch, int max_chunk,
                      bh_encoder_t** out);
void bh_encoder_destroy(bh_encoder_t* enc);
/* output geometry for chunks of L samples: T output steps, C scores per step, stride = L-per-step */
int bh_encoder_output_shape(const bh_encoder_t* enc, int L, int* T, int* C, int* stride);
/* signal: device fp16 [N][L] (the reference's [N,1,L] batch, bonito/crf/basecall.py:33).
 * scores: device fp16, contiguous [N][T][C] (the layout koi.decode.beam_search consumes). */
int bh_encoder_forward(bh_encoder_t* enc, const void* signal, int N, int L, void* scores, void* stream);
/* one text line per layer naming the kernels the engine launches for it (measurement / logging) */
int bh_encoder_describe(const bh_encoder_t* enc, char* buf, size_t bytes);
/* "lstm_exchange" (1 default: the workgroup-shared fp16 recurrent kernel hands h_t over through a small L2-resident ring
 * buffer and writes the output tensor separately; 0: through the sentinel-filled output tensor - the per-wave
 * lstm_layer_fused_kernel for H <= 512, the wide kernel's older hand-off above that; same bytes, tests).
 * "lstm_pair" (1 default: a batch of more rings than one launch of that kernel holds - more than 512 chunks at H = 384 - is served
 * two rings per workgroup on one register-resident copy of the weights, lstm_layer_wgx2_kernel; 0: one launch per 32 rings). */
/* tuning / test options (results never change): "lstm_fused" (3 default: narrowest applicable fused kernel; 2, 1, 0 = older
 * variants down to projection-by-GEMM), "lstm_force_slow" (0/1: write-through exchange), "lstm_wide" (1/0), "lstm_prefill"
 * (1 default: sentinel fill of the next recurrent layer's buffer on a side stream), "attn_ring" (1/0), "lstm_tune" (bit mask) */
int bh_encoder_set_option(bh_encoder_t* enc, const char* name, int value);
/* debug: read back the LSTM workspace (XCD agreement slots, per-wave cycle statistics when lstm_tune bit 2 is set) */
int bh_encoder_debug_read(bh_encoder_t* enc, void* host, size_t bytes, size_t offset);
/* Device-side timeouts. The persistent recurrent kernels bound every spin; a kernel that gives up raises a flag and finishes with
 * INVALID output. Flags are kept PER FORWARD: every bh_encoder_forward gets a ticket (0, 1, 2, ... per engine,
 * bh_encoder_last_ticket right after the call), zeroes its own slot in front of its kernels and ends with a 4-byte copy of the slot
 * into pinned host memory on its stream. Once the caller has observed the completion of forward `ticket` (event, decoded outputs on
 * the host, stream synchronise), bh_encoder_error_flag_at(ticket) says - without a device round trip - whether THAT forward timed
 * out; other forwards in flight are not consumed or cleared by the query (the product pipeline retries exactly the flagged batch).
 * At most 64 forwards of one engine may be in flight / unqueried (-1 for a ticket whose slot has been recycled).
 * bh_encoder_error_flag: non-zero iff any forward since the last bh_encoder_check has been SEEN to time out (host side only).
 * bh_encoder_check: synchronises `stream`, returns the same and forgets it (reference seam: bonito/crf/basecall.py:27-45 has
 * nothing that can time out; a drop-in must neither abort nor emit calls decoded from invalid scores). */
int bh_encoder_check(bh_encoder_t* enc, void* stream);
int bh_encoder_error_flag(const bh_encoder_t* enc);
long bh_encoder_last_ticket(const bh_encoder_t* enc);
int bh_encoder_error_flag_at(const bh_encoder_t* enc, long ticket);
/* The caller has handled the timeout of forward `ticket` (it re-ran the batch): forget that flag - it is then reported neither by
 * bh_encoder_error_flag / bh_encoder_check nor when its slot is recycled. 0, or -1 for a ticket whose slot has been recycled already.
 * bh_encoder_forward may run on one host thread while the four flag queries run on another (all flag state is atomic). */
int bh_encoder_ack(bh_encoder_t* enc, long ticket);

/* Per-kernel-class timing with HIP events recorded on the forward's stream (measurement only).
 * After enabling, every bh_encoder_forward appends spans; profile_read synchronises on them and returns
 * accumulated milliseconds and span counts per class, then clears. */
enum { BH_PROF_CONV = 0, BH_PROF_LSTM_GEMM = 1, BH_PROF_FILL = 2, BH_PROF_LSTM_REC = 3, BH_PROF_CRF_LINEAR = 4,
       BH_PROF_ATTENTION = 5 /* Wqkv + rotary, out_proj, the first residual norm */, BH_PROF_MLP = 6 /* fc2 + the second residual norm */,
       BH_PROF_OTHER = 7, BH_PROF_MLP_FC1 = 8 /* fc1 + SwiGLU alone: one launch per span */,
       BH_PROF_ATTENTION_CORE = 9 /* the attention kernel alone: one launch per span */, BH_PROF_CLASSES = 10 };
int bh_encoder_profile(bh_encoder_t* enc, int enable);
int bh_encoder_profile_read(bh_encoder_t* enc, float* ms /*[BH_PROF_CLASSES]*/, int* spans /*[BH_PROF_CLASSES]*/);

/* ---- CRF decode ------------------------------------------------------------------------------ */
/* Bytes of device workspace bh_crf_viterbi needs. */
size_t bh_crf_viterbi_workspace(int N, int T, int state_len);
/* Max-semiring best path (CTC_CRF.viterbi, crf/model.py:98-103).
 * scores fp16 with element strides (stride_n, stride_t); layout_5s=1: C=5S with the stay score in
 * column 5j (expand_blanks layout); layout_5s=0: C=4S koi layout + scalar blank_score.
 * moves[N][T] in {0,1}; path[N][T] in {0..4} (0 = no emission, else 1+base); best[N] path score (or NULL). */
int bh_crf_viterbi(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score,
                   long stride_n, long stride_t, void* workspace, int8_t* moves, int8_t* path,
                   float* best, void* stream);

/* CTC_CRF.reverse_complement (crf/model.py:84-96): permute scores so that decoding yields the reverse-complement
 * strand.  layout_5s=0: koi layout (stride_n = T*4S, stride_t = 4S for contiguous NTC); layout_5s=1: [T][N][5S]
 * (stride_n = 5S, stride_t = N*5S).  Out of place. */
int bh_crf_reverse_complement(const void* in, void* out, int N, int T, int state_len, int layout_5s,
                              long stride_n, long stride_t, void* stream);
/* CTC_CRF.logZ (crf/model.py:47-52), Log semiring, on contiguous koi-layout scores: logz[N] (device double).
 * workspace: bh_beam_search_workspace(N, T, state_len) bytes. */
int bh_crf_logz(const void* scores, int N, int T, int state_len, float blank_score, void* workspace, double* logz,
                void* stream);

/* ---- CTC-CRF sequence likelihood and forced alignment (csrc/seqdist.hip) ------------------------------------------
 * The chain of CTC_CRF.prepare_ctc_scores (crf/model.py:110-124): targets[N][Lmax] hold labels 1..4, 0 = padding, as int8
 * (target_bytes = 1) or int32 (target_bytes = 4); target_lengths[N] int32; all on the device. With k = state_len a row of len
 * labels is a chain of n = len + 1 - k positions, position j = the k-mer targets0[j .. j+k), targets0 = max(targets - 1, 0).
 * scores: fp16 with element strides (stride_n, stride_t) and layout_5s as in bh_crf_viterbi, so the reference's [T][N][5S]
 * tensor and the engine's [N][T][4S] tensor (+ blank_score) both go in without a copy. The stay / move edge scores are gathered
 * from the score rows inside the kernel; no [T][N][L] tensor is materialised.
 * Supported range (an error, never a truncation): 1 <= state_len <= 5, T >= 1, state_len <= Lmax, Lmax + 1 - state_len <= 4096.
 * Lengths live on the device: a row with len < state_len or len > Lmax yields NaN (callers check lengths on the host).
 * workspace: bh_crf_seq_workspace(N, T, Lmax, state_len) bytes (0 = unsupported shape), shared by the three scans below.
 *
 * bh_crf_seq_logz: koi.ctc.logZ_cu (crf/model.py:130). Log semiring, alpha_0 = [0, -inf, ...],
 *   alpha_{t+1}[j] = logaddexp(alpha_t[j] + stay_t[j], alpha_t[j-1] + move_t[j-1]); logz_out[N] = alpha_T[n-1], fp32 like the
 *   reference's scores.to(float32); -inf where n - 1 > T.
 * bh_crf_seq_viterbi: koi.ctc.viterbi_alignments (crf/model.py:143). The same scan in the Max semiring with a one-bit traceback.
 *   align_out[N][T] int32 = the chain position occupied AFTER each step: it starts from position 0 before step 0, never
 *   decreases, rises by at most 1 per step and ends at n - 1; best_out[N] = the path score. TIES RESOLVE TO STAY (a cell is
 *   entered by its move edge only when that candidate is strictly greater). A row with n - 1 > T has best = -inf and
 *   align = -1 throughout. koi is closed and the reference never calls ctc_viterbi_alignments, so the form koi returns is
 *   unknown: this compact form is this project's own definition.
 * bh_crf_seq_logz_free: the same Log scan with a FREE START, koi layout only: ln of the sum over every start state and every
 *   alignment that emits exactly the row's bases - the numerator of ln P(sequence | scores) (bh_crf_logz is the denominator).
 *   The first k emissions run through dense levels (states whose leading digits still belong to the unknown start state) in a
 *   kernel of their own, which feeds position 0 of the chain; rows shorter than state_len (0 included) are valid here.
 * bh_crf_logz_dense: CTC_CRF.logZ (crf/model.py:47-52) in fp32 for either layout with strides -> logz_out[N] float. This is what
 *   ctc_loss(normalise_scores=True) uses for the [T][N][5S] layout (a dense device scan, not a host-side expansion);
 *   bh_crf_logz serves the contiguous koi layout. */
size_t bh_crf_seq_workspace(int N, int T, int Lmax, int state_len);
int bh_crf_seq_logz(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score, long stride_n,
                    long stride_t, const void* targets, int Lmax, int target_bytes, const int32_t* target_lengths,
                    void* workspace, float* logz_out, void* stream);
int bh_crf_seq_viterbi(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score, long stride_n,
                       long stride_t, const void* targets, int Lmax, int target_bytes, const int32_t* target_lengths,
                       void* workspace, int32_t* align_out, float* best_out, void* stream);
int bh_crf_seq_logz_free(const void* scores, int N, int T, int state_len, float blank_score, long stride_n, long stride_t,
                         const void* targets, int Lmax, int target_bytes, const int32_t* target_lengths, void* workspace,
                         float* logz_out, void* stream);
int bh_crf_logz_dense(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score, long stride_n,
                      long stride_t, float* logz_out, void* stream);

/* ---- Gradients of the two log-sums above (csrc/seqdist_grad.hip): logz AND its gradient from one launch ---------------
 * The gradient of a log-sum over paths is the posterior occupancy of every edge. With alpha_t the Log scan before step t,
 * beta_t the mirror scan from beta_T[n-1] = 0 and logz = alpha_T[n-1]:
 *     p_stay[t][j] = exp(alpha_t[j]   + stay_t[j] + beta_{t+1}[j] - logz)
 *     p_move[t][j] = exp(alpha_t[j-1] + move_t[j] + beta_{t+1}[j] - logz)
 * bh_crf_seq_logz_grad: scores / targets / range exactly as bh_crf_seq_logz. grad[n][t][c] (+)= weight[n] * (sum of p over the
 *   edges whose gathered score element is c); in the koi layout the stay edge is the scalar blank_score and gets no gradient.
 *   grad: fp16 (grad_fp32 = 0) or fp32 (1) with its own element strides (g_stride_n, g_stride_t), the score axis dense, 4S or 5S
 *   wide like the scores. weight: device float [N], NULL = 1. accumulate = 1 adds into grad; accumulate = 0 writes every element
 *   of the chunk's T rows exactly once (zeros where no edge gathers). logz_out[N] is bit-identical to bh_crf_seq_logz.
 *   Positions that gather the same element at the same step (repeated k-mers) are summed before the write, in integer fixed
 *   point at scale 2^30 (a step's posteriors sum to 1), so the result is bit-identical from call to call.
 *   A row whose target cannot fit (n - 1 > T) has logz = -inf and, BY THIS PROJECT'S DEFINITION, a zero gradient (nothing added,
 *   or zeros on overwrite): koi is closed, its behaviour there is unknown, and a NaN would poison an optimiser step.
 *   A row with len < state_len or len > Lmax yields logz = NaN and no gradient is written.
 *   workspace: bh_crf_seq_grad_workspace(N, T, Lmax, state_len) bytes (every alpha_t in fp32; 0 = unsupported shape).
 * bh_crf_logz_dense_grad: the posteriors of CTC_CRF.logZ for either layout with strides (SequenceDist.posteriors, Log semiring):
 *     grad[n][t][5s'+0]   = weight[n] * exp(alpha_t[s'] + stay_t[s'] + beta_{t+1}[s'] - logZ)
 *     grad[n][t][5s'+1+r] = weight[n] * exp(alpha_t[r S/4 + s'/4] + move_t[s'][r] + beta_{t+1}[s'] - logZ)
 *   (the koi layout has the four move elements 4s'+r only). Every element of grad is written exactly once; logz_out[N] float is
 *   bit-identical to bh_crf_logz_dense. workspace: bh_crf_logz_dense_grad_workspace(N, T, state_len) bytes (0 = unsupported). */
size_t bh_crf_seq_grad_workspace(int N, int T, int Lmax, int state_len);
int bh_crf_seq_logz_grad(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score, long stride_n,
                         long stride_t, const void* targets, int Lmax, int target_bytes, const int32_t* target_lengths,
                         const float* weight, void* workspace, float* logz_out, void* grad, long g_stride_n, long g_stride_t,
                         int grad_fp32, int accumulate, void* stream);
size_t bh_crf_logz_dense_grad_workspace(int N, int T, int state_len);
int bh_crf_logz_dense_grad(const void* scores, int N, int T, int state_len, int layout_5s, float blank_score, long stride_n,
                           long stride_t, const float* weight, void* workspace, float* logz_out, void* grad, long g_stride_n,
                           long g_stride_t, int grad_fp32, void* stream);

/* ---- The CTC loss of bonito.ctc (csrc/ctc_loss.hip): torch.nn.functional.ctc_loss behind Model.ctc_label_smoothing_loss ----------
 * (bonito/ctc/model.py:48-57), with the numerator of the label-smoothing term and - in the _grad entry - the gradient, ONE launch.
 * Definition (torch's, blank = class 0): l' = the target with blanks interleaved, S = 2 len + 1 states,
 *     alpha_0[0] = lp_0[0], alpha_0[1] = lp_0[l'_1],
 *     alpha_t[s] = lp_t[l'_s] + logsumexp(alpha_{t-1}[s], alpha_{t-1}[s-1], alpha_{t-1}[s-2])   (s-2 only when l'_s != 0 and l'_s != l'_{s-2})
 *     nll = -logaddexp(alpha_{T-1}[S-1], alpha_{T-1}[S-2]);  beta = the mirror scan;
 *     occ[t][c] = sum over the states s with l'_s = c of P(the path is in s at step t | target).
 * log_probs: fp16 (logp_fp32 = 0) or fp32 (1), element strides (stride_t, stride_n), the class axis dense: [T][N][C] and [N][T][C]
 *   both go in without a copy. targets: [N][Lmax] int8 / int32 (target_bytes 1 / 4), labels 1..C-1, 0 = padding (may be NULL when
 *   Lmax = 0). target_lengths: device int32 [N].
 * nll_out[N] float. smooth_out[N] float = sum_t sum_c smooth_w[c] * lp[t][n][c] (classes with smooth_w[c] = 0 are left out), the
 *   numerator of the reference's label-smoothing term; smooth_w: device float [C]; smooth_out NULL = not computed.
 * bh_ctc_loss_grad:  grad[t][n][c] (+)= -weight[n] * occ[t][c] + smooth_weight[n] * smooth_w[c].  weight: device float [N], NULL = 1;
 *   smooth_weight: device float [N], NULL = 0 (needs smooth_w). grad: fp16 (grad_fp32 = 0) or fp32 (1) with its own element strides
 *   (g_stride_t, g_stride_n), the class axis dense. accumulate = 1 adds into grad; accumulate = 0 writes every element of the chunk's
 *   T rows exactly once. The occupancies of a step are summed in integer fixed point at scale 2^30 (they sum to 1): the result is
 *   bit-identical from call to call.
 *   THE GRADIENT IS THE TRUE DERIVATIVE of nll with respect to log_probs, -occ. torch's native ctc_loss backward returns
 *   exp(lp) - occ, the derivative with respect to the logits in front of a log_softmax; the two are identical after log_softmax's
 *   backward  g - exp(lp) * sum_c g.
 * This project's definitions where torch yields NaN:
 *   - a target that cannot fit (len + number of adjacent repeats > T), or whose every alignment crosses a -inf log-prob: nll = +inf
 *     and a ZERO gradient (nothing added, or zeros on overwrite, the smoothing term included), as in bh_crf_seq_logz_grad;
 *   - a state that a -inf log-prob makes unreachable contributes occupancy 0, not NaN;
 *   - len < 0, len > Lmax or a label outside 1..C-1 within len: nll = NaN and no gradient is written.
 * Supported range (an error, never a truncation): 2 <= C <= 8, T >= 1, N >= 1, 0 <= Lmax <= 2047; len = 0 is valid
 *   (nll = -sum_t lp_t[0]). Argument errors (range, null pointers, strides smaller than C, overlapping rows of grad) are found on the
 *   host before anything is launched.
 * workspace: bh_ctc_loss_workspace / bh_ctc_loss_grad_workspace(N, T, C, Lmax) bytes (0 = unsupported shape); the gradient keeps every
 *   alpha_t in fp32: N * T * (2 Lmax + 1 rounded up to the instance's states per thread) * 4 bytes.
 * TEST HOOK bh_ctc_loss_last_kernel: the instance (states per launch = 64 or 256 threads x states per thread; the first that holds
 *   2 Lmax + 1) that served the last call of this process, one of the codes below; 0 = none yet. Process-wide, NOT thread-safe. */
enum bh_ctc_loss_kernel {
    BH_CTC_LOSS_K_NONE = 0,
    BH_CTC_LOSS_K_W1 = 1,         /* one wave, 1 state per thread: Lmax <= 31 */
    BH_CTC_LOSS_K_W2 = 2,         /* one wave, 2: Lmax <= 63 */
    BH_CTC_LOSS_K_W4 = 4,         /* one wave, 4: Lmax <= 127 */
    BH_CTC_LOSS_K_W8 = 8,         /* one wave, 8: Lmax <= 255 */
    BH_CTC_LOSS_K_M4 = 104,       /* four waves, 4: Lmax <= 511 */
    BH_CTC_LOSS_K_M8 = 108,       /* four waves, 8: Lmax <= 1023 */
    BH_CTC_LOSS_K_M16 = 116       /* four waves, 16: Lmax <= 2047 */
};
size_t bh_ctc_loss_workspace(int N, int T, int C, int Lmax);
int bh_ctc_loss(const void* log_probs, int logp_fp32, int N, int T, int C, long stride_t, long stride_n, const void* targets,
                int Lmax, int target_bytes, const int32_t* target_lengths, const float* smooth_w, void* workspace, float* nll_out,
                float* smooth_out, void* stream);
size_t bh_ctc_loss_grad_workspace(int N, int T, int C, int Lmax);
int bh_ctc_loss_grad(const void* log_probs, int logp_fp32, int N, int T, int C, long stride_t, long stride_n, const void* targets,
                     int Lmax, int target_bytes, const int32_t* target_lengths, const float* smooth_w, const float* weight,
                     const float* smooth_weight, void* workspace, float* nll_out, float* smooth_out, void* grad, long g_stride_t,
                     long g_stride_n, int grad_fp32, int accumulate, void* stream);
int bh_ctc_loss_last_kernel(void);

/* ---- One LSTM layer for training (csrc/lstm_train.hip): the forward that keeps what the backward needs, and the backward --------
 * The layer is torch.nn.LSTM, one layer, one direction (bonito/nn.py:353-397): gates in the order i, f, g, o, h_0 = c_0 = 0,
 * insize == size == H, reverse = 1 runs the time loop backwards:
 *     a_t = x_t W_ih^T + h_{t-1} W_hh^T + b      c_t = sig(f) c_{t-1} + sig(i) tanh(g)      h_t = sig(o) tanh(c_t)
 * and from the last processed step to the first
 *     d_t = dh_t + da_{t+1} W_hh                 dc_t = dc_{t+1} sig(f_{t+1}) + d_t sig(o) (1 - tanh^2 c_t)
 *     da_t = (dc_t tanh(g) sig'(i), dc_t c_{t-1} sig'(f), dc_t sig(i) (1 - tanh^2 g), d_t tanh(c_t) sig'(o))
 *     dx_t = da_t W_ih     dW_ih = sum_t da_t^T x_t     dW_hh = sum_t da_t^T h_{t-1}     db = sum_{t,n} da_t
 * EVERY pointer is a device pointer. x, h_out / h, dh, dx: fp16 [T][N][H], 16-byte aligned. w_ih, w_hh: FP32 [4H][H]; bias: fp32 [4H]
 *   (b_ih + b_hh) or NULL. The kernels use the round-to-nearest fp16 values of the weights (converted on the device in every call:
 *   an optimiser rewrites them every step, so nothing is packed on the host); every sum is fp32, c is fp32 from step to step and
 *   where it is saved, the cell arithmetic is that of the inference kernels (lstm_cell of csrc/lstm.hip). dw_ih, dw_hh: fp32 [4H][H],
 *   dbias: fp32 [4H] or NULL = not computed; all three are OVERWRITTEN, summed in fp32 in an order that depends on the shape alone -
 *   no floating-point atomics, every output is byte-identical from call to call.
 * saved (bh_lstm_train_saved_bytes): written by the forward, read by the backward of the same T, N, H, reverse: the input projection
 *   x W_ih^T + b as fp16, overwritten in place by the post-activation gates sig(i), sig(f), tanh(g), sig(o) [T][N][4H] fp16; c [T][N][H]
 *   fp32; the fp16 weights (and scratch of the forward). workspace (bh_lstm_train_backward_workspace): da [T][N][4H] fp16, the fp16
 *   weights as the backward reads them, the partial sums of the weight gradients. Both are the caller's, 16-byte aligned; a buffer that is too small is an error.
 * Gradients are not clamped: da is stored as fp16, as autocast stores it. A non-finite dh in one chunk makes that chunk's dx and the
 *   weight gradients non-finite; the other chunks' dx keep their bytes. Chunks are independent of each other in h and dx: a chunk
 *   has the same bytes whatever else is in the batch, and whether or not N fills the last tile of 16 chunks.
 * Supported (an error with a message, never a substitute): H % 32 == 0, 32 <= H <= 1024, T >= 1, N >= 1, T * N < 2^29.
 * Stream-ordered; nothing is allocated and nothing synchronises inside. The recurrent kernels give a tile of 16 chunks to one
 *   workgroup for all T steps (bh_lstm_train_workgroups(N) of them): workgroups never wait for each other. */
size_t bh_lstm_train_saved_bytes(int T, int N, int H);               /* 0 = unsupported shape */
size_t bh_lstm_train_backward_workspace(int T, int N, int H);        /* 0 = unsupported shape */
int bh_lstm_train_workgroups(int N);
int bh_lstm_train_forward(const void* x, const float* w_ih, const float* w_hh, const float* bias, int T, int N, int H, int reverse,
                          void* h_out, void* saved, size_t saved_bytes, void* stream);
int bh_lstm_train_backward(const void* x, const float* w_ih, const float* w_hh, const void* h, const void* saved, const void* dh, int T,
                           int N, int H, int reverse, void* dx, float* dw_ih, float* dw_hh, float* dbias, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- Rotary embedding + sliding-window attention for training (csrc/attention_train.hip): the forward that keeps lse, and the backward ----
 * The attention layer of a transformer model on packed qkv (what bonito/transformer/model.py:42-79 delegates to RotaryEmbedding and
 * flash_attn_qkvpacked_func(qkv, window_size=(win_left, win_right))); key j is visible to query i of the same chunk iff
 * i - win_left <= j <= i + win_right. Per (chunk, head), rot = rotary by bh_rotary_table's angles of the token's position:
 *     q~ = fp16(rot(q) / 8)    k~ = fp16(rot(k))    s_ij = q~_i . k~_j (fp32)    lse_i = m_i + ln(sum_j exp(s_ij - m_i)) over the visible j
 *     O_i = fp16(sum_j fp16(exp(s_ij - m_i) / sum_i) V_j)
 * - the arithmetic, the kernel and the BYTES of bh_attention; lse (fp32 per chunk, head, query) is what `saved` holds. Backward, with
 * P_ij = exp(s_ij - lse_i) on the visible pairs (s recomputed by the MFMAs of the forward from the same fp16 operands) and
 * delta_i = sum_d dO_id O_id (fp32, O the stored fp16 output):
 *     dV_j = sum_i fp16(P_ij) dO_i      dP_ij = dO_i . V_j      dS_ij = fp16(P_ij (dP_ij - delta_i))
 *     dq~_i = sum_j dS_ij k~_j          dk~_j = sum_i dS_ij q~_i
 *     dq = rot^-1(dq~) / 8              dk = rot^-1(dk~)         (rot^-1 = rotation by the negated angle)
 * q~, k~, P and dS are fp16 MFMA operands; every sum and everything else is fp32; dq, dk, dv are rounded once, at the store. Upstream
 *   gradients arrive loss-scaled; nothing is scaled or clamped here.
 * EVERY pointer is a device pointer, 16-byte aligned. qkv, dqkv: fp16 [N*T][3*nhead*64] (q | k | v, head-major inside each); out, dout:
 *   fp16 [N*T][nhead*64]; cos_sin: device copy of bh_rotary_table(T, 64). dqkv is OVERWRITTEN, every element of it.
 * No floating-point atomics and no order that depends on scheduling: a query pass owns dq of its 128 queries, a key pass owns dk and dv of
 *   its 128 keys (the window mirrored), both recompute S as the forward did. Two calls give equal bytes; chunks are independent.
 * saved (bh_attention_train_saved_bytes): lse, written by the forward, read by the backward of the same N, T, nhead and window.
 *   workspace (bh_attention_train_backward_workspace): delta. Both are the caller's; a buffer that is too small is an error.
 * Supported (an error with a message, never a substitute, nothing launched, outputs untouched): head_dim == 64, win_left, win_right >= 0
 *   with (16 + win_left + win_right + 15) / 16 <= 26 (what bh_attention serves), N, T, nhead >= 1, N, nhead <= 65535.
 * Stream-ordered; nothing is allocated and nothing synchronises inside. */
size_t bh_attention_train_saved_bytes(int N, int T, int nhead);                                       /* 0 = unsupported */
size_t bh_attention_train_backward_workspace(int N, int T, int nhead, int win_left, int win_right);   /* 0 = unsupported window */
int bh_attention_train_forward(const void* qkv, const float* cos_sin, int N, int T, int nhead, int head_dim, int win_left, int win_right,
                               void* out, void* saved, size_t saved_bytes, void* stream);
int bh_attention_train_backward(const void* qkv, const float* cos_sin, const void* out, const void* saved, const void* dout,
                                int N, int T, int nhead, int head_dim, int win_left, int win_right,
                                void* dqkv, void* workspace, size_t workspace_bytes, void* stream);

/* ---- The convolution and the linear / CRF-head layer for training (csrc/train_layers.hip): forward on the rounded master weights, backward ----
 * With bh_lstm_train_* and bh_crf_seq_logz_grad these are all layers of an LSTM-family CRF model (SeqdistModel.forward_train).
 * Arithmetic (that of autocast training, as for the LSTM layer): activations and their gradients are fp16; w and bias are fp32 DEVICE
 *   tensors in torch's layout, rounded to nearest fp16 on the device in every call; every sum is fp32; dw and db are fp32 and
 *   OVERWRITTEN. No floating-point atomics: the rows are split into blocks by a rule of the shape alone and the partial sums are added
 *   in block order, so two calls give equal bytes.
 * Convolution: x fp16 [N][Lin][Cin] channel-minor ([N][Lin] for Cin == 1), w [Cout][Cin][K], y = clamp(act(conv(x, w) + bias), lo, hi)
 *   written at n * os_n + t * os_t + c (os_n = Cout, os_t = N * Cout stores time-major [T][N][C]), Lout = (Lin + 2 pad - K) / stride + 1.
 *   forward: y has the bytes of bh_conv1d_first / bh_conv1d on the same rounded weights and bias; the workspace then BEGINS with the
 *   weights as those kernels read them (Cin > 1: the bytes of bh_conv1d_pack, bh_conv1d_packed_halves halves; Cin == 1: fp32 [Cout][K]).
 *   backward, dy in the layout of y:  dz = dy * m * act'(z) stored as fp16, m = [lo < y < hi] read from the STORED y (strictly inside;
 *   m = 1 for lo = -inf, hi = +inf), act' at z recomputed in fp32 from x and the rounded weights;  db[c] = sum dz;
 *   dw[co][ci][k] = sum_{n,t} dz[n][t][co] x[n][t s - p + k][ci];  dx[n][l][ci] = sum_{co,k: (l+p-k) mod s = 0} w[co][ci][k] dz[n][(l+p-k)/s][co]
 *   as fp16 in the layout of x. dx and db may be NULL = not computed.
 *   Supported: Cin == 1 or Cin % 8 == 0, Cout % 4 == 0, K <= 32, stride <= 8, pad < K, Lin + 2 pad >= K, os_n and os_t multiples of 4.
 * Linear: x fp16 [M][K] with rows m = t * N + n, w [C][K], Y = clamp(act(x w^T + bias) * scale, lo, hi), act none or tanh;
 *   batch_major = 1 stores Y as [N][T][C] (the engine's row remap, what bh_encoder_forward returns), 0 as [T][N][C].
 *   forward: the bytes of bh_linear on the rounded weights.  backward, dy in the layout of Y:  dZ[m][c] = dy * m * scale * act' as fp16,
 *   m from the stored Y, tanh' = 1 - (Y / scale)^2 from the stored Y;  dx = dZ w (fp16, through bh_linear on the transposed rounded
 *   weights), dw = dZ^T x, db = sum dZ. dx and db may be NULL. A fixed blank column (expand_blanks) is never materialised.
 *   Supported: K % 8 == 0, C % 8 == 0, T * N < 2^31; T * N * C may pass 2^31 elements (64-bit offsets throughout).
 * workspace (bh_*_train_workspace, one size for forward and backward of a shape; 0 = unsupported shape): the caller's, 16-byte aligned.
 * Anything unsupported returns nonzero with bh_last_error() set, launches nothing and leaves every output untouched.
 * Stream-ordered; nothing is allocated and nothing synchronises inside. */
size_t bh_conv1d_train_workspace(int N, int Lin, int Cin, int Cout, int K, int stride, int pad);
int bh_conv1d_train_forward(const void* x, const float* w, const float* bias, int N, int Lin, int Cin, int Cout, int K, int stride, int pad,
                            int act, float clamp_lo, float clamp_hi, long os_n, long os_t, void* y, void* workspace, size_t workspace_bytes,
                            void* stream);
int bh_conv1d_train_backward(const void* x, const float* w, const float* bias, const void* y, const void* dy, int N, int Lin, int Cin, int Cout,
                             int K, int stride, int pad, int act, float clamp_lo, float clamp_hi, long os_n, long os_t, void* dx, float* dw,
                             float* db, void* workspace, size_t workspace_bytes, void* stream);
size_t bh_linear_train_workspace(int T, int N, int K, int C);
int bh_linear_train_forward(const void* x, const float* w, const float* bias, int T, int N, int K, int C, int act, float scale,
                            float clamp_lo, float clamp_hi, int batch_major, void* y, void* workspace, size_t workspace_bytes, void* stream);
int bh_linear_train_backward(const void* x, const float* w, const void* y, const void* dy, int T, int N, int K, int C, int act, float scale,
                             float clamp_lo, float clamp_hi, int batch_major, void* dx, float* dw, float* db, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- What a transformer encoder layer adds to training (csrc/transformer_train.hip): the norm's backward, and fc1 + SwiGLU ----------
 * With bh_attention_train_* and bh_linear_train_* these are all pieces of a TransformerEncoderLayer (bonito/transformer/model.py:83-133:
 * x1 = norm1(attn(x) + alpha x), out = norm2(ff(x1) + alpha x1); bonito_amd.attn.encoder_layer chains them).
 * DeepNorm residual RMSNorm, a, x, dy fp16 [M][D], w fp32 [D] (used as it is, as bh_rmsnorm_residual does):
 *     z = a + alpha x      r = rsqrt(mean_d z^2 + eps)      out = fp16(z r w)             - the forward IS bh_rmsnorm_residual; nothing is saved
 *   backward, z and r recomputed from a and x:
 *     g = dy w      c = (1/D) sum_d g_d z_d      dz = r g - r^3 c z
 *     da = fp16(dz)      dx = fp16(alpha dz)      dw[d] = sum_m dy[m][d] z[m][d] r[m]   (fp32, OVERWRITTEN)
 *   Every sum and every intermediate is fp32; da and dx are rounded once, at the store. dy arrives loss-scaled; nothing is scaled or
 *   clamped. da or dx may be NULL = not written. One wave per row; dw: a workgroup sums a block of rows (the block a function of M
 *   alone) into the workspace and a second launch adds the blocks in block order (eight runs of consecutive blocks, each added in block
 *   order, then the runs in order) - no floating-point atomics, two calls give equal bytes.
 *   Supported: D a multiple of 8 in 8..1024, M >= 1.
 * Gated input layer of the MLP, x fp16 [M][D], w fp32 [2F][D] in torch's layout (y rows first, then gate rows: flash-attn's GatedMlp):
 *     [y | gate] = x fp16(w)^T      h = fp16(y gate sigmoid(gate))     fp16 [M][F]
 *   forward: the weights are rounded and their rows interleaved (y_j, gate_j) on the device, then bh_linear's gated epilogue runs: h has
 *   the bytes of bh_linear(gated = 1) on those weights, which is what bh_encoder_forward computes.
 *   backward, from dh fp16 [M][F]: u = [y | gate] is RECOMPUTED by the plain GEMM and stored as fp16 (the forward keeps nothing), then
 *     s = sigmoid(gate)      dy = dh gate s      dgate = dh y s (1 + gate (1 - s))      du = fp16([dy | dgate])   (fp32, one rounding)
 *     dx = du fp16(w) (fp16, through bh_linear on the transposed rounded weights)      dw = du^T x (fp32 [2F][D], torch's row order, OVERWRITTEN)
 *   dx may be NULL. dw's reduction over rows is that of bh_linear_train_backward: equal bytes from call to call.
 *   Supported: D % 8 == 0, F % 8 == 0, M < 2^31; M * 2F may pass 2^31 elements (64-bit offsets throughout).
 * EVERY pointer is a device pointer, 16-byte aligned. workspace (bh_*_train_workspace; 0 = unsupported shape): the caller's.
 * Anything unsupported returns nonzero with bh_last_error() set, launches nothing and leaves every output untouched.
 * Stream-ordered; nothing is allocated and nothing synchronises inside. */
size_t bh_rmsnorm_train_workspace(long M, int D);
int bh_rmsnorm_train_backward(const void* a, const void* x, const float* w, const void* dy, long M, int D, float alpha, float eps,
                              void* da, void* dx, float* dw, void* workspace, size_t workspace_bytes, void* stream);
size_t bh_gated_linear_train_workspace(long M, int D, int F);
int bh_gated_linear_train_forward(const void* x, const float* w, long M, int D, int F, void* h, void* workspace, size_t workspace_bytes,
                                  void* stream);
int bh_gated_linear_train_backward(const void* x, const float* w, const void* dh, long M, int D, int F, void* dx, float* dw,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- Batch-statistics BatchNorm for training (csrc/batchnorm_train.hip): what follows conv(x) in a normalised convolution ------------
 * torch.nn.BatchNorm1d in training mode with the activation and the clamp of the convolution (bonito/nn.py Convolution.forward:
 * activation(norm(conv(x)))); bh_conv1d_train_forward with act none and no clamp yields z. M = N L rows per channel:
 *     mean_c = (1/M) sum z      var_c = (1/M) sum (z - mean_c)^2 (biased)      rstd_c = 1 / sqrt(var_c + eps)
 *     xh = (z - mean_c) rstd_c      u = gamma_c xh + beta_c      y = fp16(clamp(act(u), lo, hi))
 *   z fp16 [N][L][C] channel-minor; y written at n * os_n + t * os_t + c (os_n = C, os_t = N * C stores time-major [L][N][C]).
 *   gamma, beta fp32 [C_param], used unrounded; both NULL = affine off (1 and 0). mean and rstd: fp32 [C_param] outputs, the
 *   backward's inputs. running_mean / running_var fp32 [C_param], updated in place by the finishing kernel (no host synchronisation):
 *     rm <- (1 - momentum) rm + momentum mean      rv <- (1 - momentum) rv + momentum var M / (M - 1);     both NULL = not tracked.
 *   C_param <= C counts the real channels: channels c >= C_param (zero padding up to a multiple of 8) get y = 0 and dz = 0 exactly, and
 *   no statistic, parameter or gradient is read or written for them.
 *   Every sum is fp32. A workgroup sums a block of rows (the block a function of M alone), a thread every k-th row of it in row order;
 *   the threads of a workgroup are added in a fixed order through LDS and the blocks in block order by a second launch - no
 *   floating-point atomics, two calls give equal bytes. The variance is the CENTRED sum of a second pass over z, never E[z^2] - E[z]^2.
 *   backward, dy in the layout of y, dz fp16 [N][L][C] in z's row order:
 *     du = dy [lo < y < hi] act'(u)   (u recomputed in fp32 from z, mean, rstd; the mask from the STORED y, strictly inside)
 *     dbeta_c = sum du      dgamma_c = sum du xh      dz = fp16(gamma_c rstd_c (du - dbeta_c / M - xh dgamma_c / M))
 *   dgamma and dbeta fp32 [C_param], OVERWRITTEN; either may be NULL = not written.
 *   Supported: N L >= 2 (more than one value per channel), C a multiple of 8 up to 2048, 1 <= C_param <= C, act none / swish / tanh /
 *   relu, os_n and os_t multiples of 8, eps > 0, 0 <= momentum <= 1; N L C may pass 2^31 elements (64-bit offsets throughout).
 * z, y, dy, dz and the workspace are 16-byte aligned device pointers. workspace (bh_batchnorm_train_workspace, one size for forward and
 * backward; 0 = unsupported shape): the caller's. Anything unsupported returns nonzero with bh_last_error() set, launches nothing and
 * leaves every output untouched. Stream-ordered; nothing is allocated and nothing synchronises inside. */
size_t bh_batchnorm_train_workspace(int N, int L, int C);
int bh_batchnorm_train_forward(const void* z, const float* gamma, const float* beta, float* running_mean, float* running_var, int N, int L,
                               int C, int C_param, float eps, float momentum, int act, float clamp_lo, float clamp_hi, long os_n, long os_t,
                               void* y, float* mean, float* rstd, void* workspace, size_t workspace_bytes, void* stream);
int bh_batchnorm_train_backward(const void* z, const float* gamma, const float* beta, const float* mean, const float* rstd, const void* y,
                                const void* dy, int N, int L, int C, int C_param, int act, float clamp_lo, float clamp_hi, long os_n,
                                long os_t, void* dz, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Training a QuartzNet CTC model (csrc/quartznet_train.hip): depthwise backward, residual + activation + dropout, head backward ---
 * Depthwise convolution, stride 1, dilation 1. The forward is bh_dwconv1d as it stands (fp32 weights unrounded, fmaf over the taps in tap
 * order, one rounding at the store). x fp16 [N][L][C] channel-minor, w fp32 [C][K], dy fp16 [N][Lout][C], Lout = L + 2 pad - K + 1:
 *     dx[n][p][c] = fp16(sum_k w[c][k] dy[n][p + pad - k][c])      over the k with 0 <= p + pad - k < Lout, fp32 fmaf in tap order
 *     dw[c][k]    = sum_{n,t} dy[n][t][c] x[n][t + k - pad][c]      fp32 [C][K], OVERWRITTEN; terms with the x index outside 0..L-1 are 0
 *   dx or dw may be NULL = not written. dw: a workgroup owns 64 channels and a block of consecutive units of 64 rows (the block a function
 *   of the shape alone), a thread fixed (channel, tap) accumulators added to in row order; the [block][C][K] planes lie in the workspace
 *   and a second launch adds them in block order (eight runs of consecutive blocks, each in block order, then the runs in order) - no
 *   floating-point atomics, two calls give equal bytes.
 *   Supported: C % 8 == 0, 1 <= K <= 127, 0 <= pad < K, Lout >= 1, N L < 2^30 rows; N L C may pass 2^31 elements (64-bit offsets).
 * Residual add + activation + dropout, a, b, y, dy, da fp16 [M][C] (M = N L rows, C % 8 == 0), b may be NULL (u = a):
 *     u = a + b (fp32)      y = fp16(keep ? act(u) inv_keep : 0)      da = fp16(keep ? dy inv_keep act'(u) : 0)   (u recomputed)
 *   da is the gradient of b as well. act: none / swish / tanh / relu, the functions of the other training layers. keep is NOT stored: with
 *   64-bit unsigned arithmetic (mod 2^64), G = 0x9E3779B97F4A7C15 and the splitmix64 finaliser
 *     mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *     keep(i) = (mix(mix(seed + G (stream_id + 1)) + G (i + 1)) >> 32) >= p_threshold          i = m C + c, the flat element index
 *   The host computes p_threshold = floor(p 2^32) in double and inv_keep = (float)(1 / (1 - p)), 0 <= p < 1. p = 0: p_threshold = 0 keeps
 *   every element and inv_keep = 1, the bytes are those of fp16(act(a + b)). M C < 2^35 elements.
 * CTC head, x fp16 [M][F], w fp32 [classes][F], bias fp32 [classes]. The forward is bh_ctc_head as it stands. Backward from dlp fp16
 * [M][classes], the gradient of the log-probabilities:
 *     logit, s = softmax(logit): RECOMPUTED in fp32 from x, w, bias exactly as the forward forms them (never from the rounded output)
 *     dlogit_c = dlp_c - s_c sum_{c' < classes} dlp_c'      dx = fp16(sum_c dlogit_c w[c][.])  (fmaf in class order)
 *     dw[c][f] = sum_m dlogit[m][c] x[m][f]      db[c] = sum_m dlogit[m][c]      fp32, OVERWRITTEN
 *   dx, dw, db may each be NULL = not written. dlogit is kept as fp32 [M][8] in the workspace; dw and db: a workgroup sums a block of rows
 *   (a function of M alone) in row order, the blocks are added in block order - equal bytes from call to call.
 *   Supported: 1 <= classes <= 8, F % 8 == 0, classes F fp32 weights within 64 KiB of LDS, M < 2^32.
 * x, dy, dx, a, b, y, da and the workspace are 16-byte aligned device pointers. workspace (bh_*_train_workspace; 0 = unsupported shape):
 * the caller's. Anything unsupported returns nonzero with bh_last_error() set, launches nothing and leaves every output untouched.
 * Stream-ordered; nothing is allocated and nothing synchronises inside. */
size_t bh_dwconv1d_train_workspace(int N, int L, int C, int K, int pad);
int bh_dwconv1d_train_backward(const void* x, const float* w, const void* dy, int N, int L, int C, int K, int pad, void* dx, float* dw,
                               void* workspace, size_t workspace_bytes, void* stream);
int bh_residual_act_train_forward(const void* a, const void* b, long M, int C, int act, unsigned int p_threshold, float inv_keep,
                                  unsigned long long seed, unsigned long long stream_id, void* y, void* stream);
int bh_residual_act_train_backward(const void* a, const void* b, const void* dy, long M, int C, int act, unsigned int p_threshold,
                                   float inv_keep, unsigned long long seed, unsigned long long stream_id, void* da, void* stream);
size_t bh_ctc_head_train_workspace(long M, int F, int classes);
int bh_ctc_head_train_backward(const void* x, const float* w, const float* bias, const void* dlp, long M, int F, int classes, void* dx,
                               float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Smith-Waterman local alignment with affine gaps and a traceback (csrc/align.hip) ----------------------------------
 * n pairs of a called sequence `seq` (the query, index i) and a known sequence `ref` (index j). seqs / refs: DEVICE int8 planes
 * [n][stride] of the codes 1..4 (decode.encode_sequences), 0 = padding. seq_lengths / ref_lengths: HOST int32 [n] (they are
 * validated before anything is launched, then copied into the workspace). Exact int32 scores, a gap of length k costs
 * gap_open + (k - 1) * gap_extend:
 *     E(i,j) = max(H(i,j-1) - open, E(i,j-1) - extend)     deletion, CIGAR D        F(i,j) = max(H(i-1,j) - open, F(i-1,j) - extend)
 *     H(i,j) = max(0, H(i-1,j-1) + (seq_i == ref_j ? match : mismatch), E(i,j), F(i,j))                         insertion, CIGAR I
 * End cell: the largest H, among equals the smallest i, then the smallest j. Traceback in H: stop at H = 0, else prefer the
 * diagonal, then E, then F; in E / F the open wins a tie with the extension.
 * result: DEVICE int32 [n][10] = score, num_correct (=), num_mismatches (X), num_insertions (I), num_deletions (D),
 *   align_ref_start, align_ref_end, align_seq_start, align_seq_end (0-based, ends inclusive), number of CIGAR runs.
 *   A pair with score 0 (an empty sequence among them): counts 0, starts 0, ends -1, no runs.
 * ops (optional, DEVICE uint32 [n][ops_stride]) with n_ops (optional, DEVICE int32 [n]): the run-length CIGAR in alignment order,
 *   one run = (length << 2) | op, op 0 '=', 1 'X', 2 'I', 3 'D'. ops_stride must hold the longest CIGAR any pair could have
 *   (seq_len + ref_len - 1 runs; 0 for an empty pair): a shorter buffer is an error, never a truncated CIGAR.
 * workspace: DEVICE, bh_sw_workspace(n, max seq length, max ref length) bytes (0 = unsupported shape: n < 1 or a length outside
 *   0..4096); 4 traceback bits per cell: n * ceil(max_seq / 512) * (max_ref + 63) * 256 bytes plus a small head.
 * Errors (non-zero, bh_last_error() set, nothing launched): negative lengths, a length beyond its stride or beyond 4096,
 *   match < 1, mismatch >= match, gap_extend < 1, gap_open < gap_extend, a parameter beyond 32767 in magnitude, a workspace or
 *   ops buffer that is too small. */
size_t bh_sw_workspace(int n, int max_seq, int max_ref);
int bh_sw_align(const void* seqs, long seq_stride, const int32_t* seq_lengths, const void* refs, long ref_stride,
                const int32_t* ref_lengths, int n, int match, int mismatch, int gap_open, int gap_extend, void* workspace,
                size_t workspace_bytes, int32_t* result, uint32_t* ops, long ops_stride, int32_t* n_ops, void* stream);

/* Semi-global mode of the affine aligner: parasail.sg_trace_scan_32(query, ref, 10, 2, dnafull) behind the reference's duplex end
 * repair (bonito/cli/duplex.py:240-243). The recurrences of bh_sw_align without the floor at 0; H(i,0) = H(0,j) = 0 (end gaps are free
 * on both sequences at both ends), E and F start at minus infinity. End cell: the largest H over the last row and the last column,
 * among equals the smallest i, then the smallest j. Traceback: the diagonal, then E, then F; in E / F the open wins a tie; it stops on
 * reaching row 0 or column 0. The CIGAR covers BOTH sequences completely: what lies before the first and after the last aligned
 * column comes out as one I (seq) or D (ref) run each, merged with an equal neighbour. Arguments, workspace (bh_sw_workspace), limits
 * and errors as bh_sw_align, except: ops_stride must hold seq_len + ref_len runs; the counts of the result row include the overhang
 * runs, the four start / end columns describe the aligned part; a pair with an empty sequence has score 0 and a single I or D run
 * over the other one (no run when both are empty), starts 0 and ends -1. The score may be negative. */
int bh_sg_align(const void* seqs, long seq_stride, const int32_t* seq_lengths, const void* refs, long ref_stride,
                const int32_t* ref_lengths, int n, int match, int mismatch, int gap_open, int gap_extend, void* workspace,
                size_t workspace_bytes, int32_t* result, uint32_t* ops, long ops_stride, int32_t* n_ops, void* stream);

/* Banded global alignment under unit costs with a traceback: edlib.align(query, ref, task="path") behind the reference's duplex caller
 * (bonito/cli/duplex.py:246-248). n pairs, one wave per pair, sequences of up to 65536 bases, arguments as bh_sw_align.
 *   D(0,0) = 0, D(i,0) = i, D(0,j) = j
 *   D(i,j) = min(D(i-1,j-1) + [seq_i != ref_j], D(i,j-1) + 1 (D: consumes a ref base), D(i-1,j) + 1 (I: consumes a seq base))
 *   Traceback from (m,n): among the predecessors that attain the minimum the diagonal first, then D, then I.
 * k (1..65536) is the band's half-width: with delta = ref_len - seq_len only the cells whose diagonal j - i lies in
 *   [min(0, delta) - k, max(0, delta) + k] are computed, every other cell counts as +infinity. A pair is ACCEPTED when its banded
 *   distance d satisfies floor((d - |delta|) / 2) <= k; distance and CIGAR then equal those of the full matrix. A rejected pair is to
 *   be run again with a larger k (the caller's loop: align.nw_align doubles it).
 * result (DEVICE int32 [n][8]): distance, counts of = X I D, number of runs, k, status. status 0: accepted. status 1: rejected, the
 *   band was too narrow: distance is an upper bound, counts and runs are 0, no ops are written.
 * ops / n_ops as bh_sw_align; ops_stride must hold seq_len + ref_len runs. A pair with an empty sequence has a single I or D run.
 * workspace: DEVICE, bh_nw_workspace(n, max seq length, max ref length, max_band) bytes, max_band = the largest
 *   |ref_len - seq_len| + 2 k + 1 of the batch (0 = unsupported shape). 2 traceback bits per cell of a pass's band window:
 *   n * ceil(max_seq / 512) * (min(max_ref, 511 + max_band) + 63) * 128 bytes plus a small head; never seq * ref. */
size_t bh_nw_workspace(int n, int max_seq, int max_ref, long max_band);
int bh_nw_align(const void* seqs, long seq_stride, const int32_t* seq_lengths, const void* refs, long ref_stride,
                const int32_t* ref_lengths, int n, int k, void* workspace, size_t workspace_bytes, int32_t* result, uint32_t* ops,
                long ops_stride, int32_t* n_ops, void* stream);

/* The read mapper ("Mapper"): what `bonito basecaller --reference` gets from mappy / minimap2 (bonito/aligner.py),
 * DEFINED by the restatement tests/mapper_ref.py, not by minimap2: seeds, chain scores, mapq and tie-breaks are this project's.
 * Three steps on the device; sorting and the prefix sums between them are the caller's; the base alignment is bh_nw_align.
 *
 * bh_map_sketch: the (k, w)-minimizers of n sequences, 11 <= k <= 28, 1 <= w <= 64.
 *   codes (DEVICE int8 [n][stride]): 1..4 = A C G T, anything else = no base (padding behind a sequence included); lengths: HOST.
 *   The k-mer ending at p has the 2k-bit values fw (first base in the top bits) and rv (its reverse complement); its key is the smaller
 *   of mix(fw), mix(rv) (mix: the seven-step invertible map spelt out in tests/mapper_ref.py), the strand bit says that mix(rv) was the
 *   smaller; a k-mer with a non-base, or with mix(fw) = mix(rv), has no key. The window ending at p holds the k-mer ends
 *   max(k - 1, p - w + 1) .. p; windows end at every p >= min(k + w - 2, len - 1); a window selects the leftmost of its smallest keys.
 *   Output (DEVICE): keys[o], pos[o] (the k-mer's last base), strand[o] for the distinct selected positions of sequence 0 in position
 *   order, then those of sequence 1, ...; offsets (int32 [n + 1]): where each sequence's minimizers start, offsets[n] = their number.
 *   capacity: entries in keys / pos / strand; at least sum(max(0, len - k + 1)), one per k-mer (an error otherwise, never truncation).
 *   workspace: DEVICE, bh_map_sketch_workspace(n, sum of the lengths) bytes (0 = unsupported). A workgroup covers
 *   bh_map_sketch_tile() window ends of one sequence. With n = 1 the stride is not read (a contig inside a longer buffer).
 *   Errors (rc != 0): k or w out of range, a negative length, a length beyond the stride, lengths that total 2^31 or more, an output
 *   or workspace that is too small.
 * bh_map_seed: one anchor per (query minimizer, occurrence of its key in the index), for the n <= 1024 reads of one sketch call.
 *   Query side: keys / pos / strand / offsets as bh_map_sketch wrote them, n_min = offsets[n] (HOST), q_lengths (DEVICE int32 [n]).
 *   Index side (DEVICE): ukeys (the distinct keys, increasing), ustart / ucount (the run of each key in rpos / rstrand), rpos (position
 *   of the k-mer's last base in the concatenated reference, below 2^31) and rstrand, sorted by (key, rpos). A key with more than
 *   max_occ occurrences gives no anchor.
 *   Called with offsets = NULL it writes counts[q], the anchors of query minimizer q; called again with their exclusive prefix sums in
 *   offsets (int64 [n_min]) it writes anchors[offsets[q] + j] = read << 53 | strand << 52 | rpos << 21 | qpos', strand = query strand xor
 *   reference strand, qpos' = qpos, on strand 1 q_length - qpos + k - 2 (the same k-mer's last base on the reverse-complemented
 *   read; reads of fewer than 2^21 bases). Sorting these words sorts by (read, strand, contig, rpos, qpos'). Nothing beyond capacity
 *   is written.
 * bh_map_chain: the chaining DP, the primary chain and s2 for n <= 1024 reads, one wave per read.
 *   anchors: the sorted words; contigs (int32 per anchor): the contig of rpos; offsets (int32 [n + 1]): each read's anchors.
 *   f[i] = max(k, max_j f[j] + min(dq, dr, k) - cost(|dr - dq|)) over j = i - 64 .. i - 1 of the same read, strand and contig with
 *   0 < dq <= max_dist, 0 < dr <= max_dist, |dr - dq| <= bandwidth; cost(0) = 0, cost(g) = ((5 g) >> 5) + (floor(log2 g) >> 1). A
 *   predecessor is taken only when its score exceeds k, among equal scores the largest j. p[i]: the predecessor (index within the
 *   read) or -1. The chain ends at the largest f, among equals the smallest index; chain (int32, the read's slice): its anchors from
 *   the LAST to the first. result (int32 [n][4]): anchors in the chain, s1 (its f), s2 (the largest f on another strand or contig or
 *   with rpos outside the chain's [first, last] rpos; 0 if none), index of the end anchor (0, 0, 0, -1 for a read without anchors).
 *   Errors: n, k, max_dist or bandwidth out of range, 2^31 anchors or more. */
int bh_map_sketch_tile(void);
size_t bh_map_sketch_workspace(int n, long total_len);
int bh_map_sketch(const void* codes, long stride, const int32_t* lengths, int n, int k, int w, void* workspace, size_t workspace_bytes,
                  int64_t* keys, int32_t* pos, int8_t* strand, long capacity, int32_t* offsets, void* stream);
int bh_map_seed(const int64_t* qkeys, const int32_t* qpos, const int8_t* qstrand, const int32_t* q_offsets, const int32_t* q_lengths,
                int n, long n_min, const int64_t* ukeys, const int32_t* ustart, const int32_t* ucount, long n_ukeys,
                const int32_t* rpos, const int8_t* rstrand, int k, int max_occ, int32_t* counts, const int64_t* offsets,
                int64_t* anchors, long capacity, void* stream);
int bh_map_chain(const int64_t* anchors, const int32_t* contigs, const int32_t* offsets, int n, long n_anchors, int k, int max_dist,
                 int bandwidth, int32_t* f, int32_t* p, int32_t* chain, int32_t* result, void* stream);

/* bh_map_extend: end extension of mappings beyond their outermost anchors (`Aligner(extend_ends=True)`, `basecaller --extend-ends` and
 * `--save-ctc`), DEFINED by tests/mapper_ext_ref.py and equal to it bit for bit. One wave per end, all arrays DEVICE arrays.
 *   reads (int8 [n_reads][stride]): the read codes as given, 1..4 = A C G T, anything else = no base; read_len (int32 [n_reads]).
 *   ref (int8 [ref_len]): the concatenated reference codes, ref_len < 2^31.
 *   ends (int32 [n_ends][6]): read row, strand (0 / 1), side (0 = left, 1 = right), the span's start (left) or end (right) on the
 *   ALIGNED strand of the read (on strand 1 the base at p is the complement of reads[row][len - 1 - p]), the same in the concatenated
 *   reference, and the contig's limit on that side (left: its first base; right: one behind its last): a tail never leaves its contig.
 *   Tails (nearest base first): Q = the up to bh_map_extend_max() = 512 query bases beyond the span, R = the up to
 *   len(Q) + bh_map_extend_band() = len(Q) + 32 reference bases. S(0,0) = 0; only cells with |j - i| <= 32 exist;
 *   S(i,j) = max(S(i-1,j-1) + (Q[i-1] == R[j-1], a base of ACGT ? +2 : -4), S(i-1,j) - 4, S(i,j-1) - 4). End cell: the largest S, (0,0)
 *   included, then the smallest i + j, then the smallest i. Path back to (0,0): diagonal, then (i-1,j) (I), then (i,j-1) (D). There
 *   is no drop-off heuristic; tails beyond 512 bases stay clipped.
 *   result (int32 [n_ends][4]): score, query bases, reference bases, number of runs; (0, 0, 0, -1) for an end that does not fit its
 *   read, its contig limit or the reference (nothing of it is read). runs (uint32 [n_ends][runs_cap]): count << 2 | op over
 *   = X I D = 0 1 2 3 in READ order at both sides (left runs + the span's runs + right runs is the whole alignment);
 *   runs_cap >= 2 * 512 + 32. Nothing else of result / runs is written.
 *   Errors: a null pointer, n_ends < 0, runs_cap too small, a negative count or stride. n_ends == 0 returns 0 without a launch. */
int bh_map_extend_max(void);
int bh_map_extend_band(void);
int bh_map_extend(const int8_t* reads, long stride, const int32_t* read_len, int n_reads, const int8_t* ref, long ref_len,
                  const int32_t* ends, int n_ends, int32_t* result, uint32_t* runs, int runs_cap, void* stream);

/* Signal ingest on the device: replaces Read.__init__'s numpy work (bonito/reader.py:122-166 normalisation + trim, the pA
 * scaling and the trim threshold of bonito/pod5.py:52-67) and util.chunk + the fp16 cast (bonito/util.py:142-161, crf/basecall.py:31) for raw
 * int16 reads, with the reference's arithmetic reproduced bit for bit. All pointers are device pointers.
 *   raw: concatenated int16 samples of n_reads reads, offsets[n_reads + 1]; cal_scale / cal_offset: per-read calibration
 *   (pA = cal_scale * (raw + cal_offset)); strategy 0 = quantile scaling with (quantile_a, quantile_b, shift_mult,
 *   scale_mult), 1 = fixed pA (fixed_shift, fixed_scale). Outputs per read: shift, scale (fp64), weak (bit0: shift is the
 *   literal 10, bit1: scale is the literal 1.0, bit2: fixed pA, both are config floats -- NumPy's promotion then keeps the
 *   arithmetic in fp32 with the constants rounded to fp32), trim (first sample of the read proper).
 * bh_signal_chunks writes normalised fp16 rows [n_chunks][chunk_samples]: row i = read chunk_read[i], samples
 *   chunk_start[i] .. (chunk_len[i] >= chunk_samples) or the chunk_len[i] available samples tiled (short reads). */
int bh_signal_normalise(const int16_t* raw, const long* offsets, const float* cal_scale, const float* cal_offset, int n_reads,
                        int strategy, double quantile_a, double quantile_b, double shift_mult, double scale_mult,
                        double fixed_shift, double fixed_scale, int do_trim, double* shift, double* scale, int* weak, int* trim,
                        void* stream);
int bh_signal_chunks(const int16_t* raw, const long* offsets, const float* cal_scale, const float* cal_offset,
                     const double* shift, const double* scale, const int* weak, const int* chunk_read, const long* chunk_start,
                     const long* chunk_len, int n_chunks, int chunk_samples, void* out, void* stream);

/* Operator level (parity tests): one recurrent layer of the 8-bit path Q8-1 (koi's `quantize`, bonito/crf/model.py:245; the
 * arithmetic is defined in oracle/lstm_q8_ref.py) from fp32 HOST weights W_ih, W_hh [4H][H] and bias [4H] (b_ih + b_hh, or NULL).
 * x: device fp16 [T][N][H], N % 16 == 0, quantised with the static scale 127 / bound; h16_out (or NULL): device fp16 [T][N][H];
 * hq_frag (or NULL): device int8 output in MFMA fragment order [T][N/16][ceil(H/64)][64][16] (padding units of the last k-step,
 * H % 64 != 0, are not written); sums (or NULL): device int32 [T][N][4H][2] = the exact integer sums (input part, recurrent part)
 * per gate row. The outputs choose the kernel instance the way the engine does: sums -> the debug instance (needs h16_out); else
 * h16_out -> the last recurrent layer's; hq_frag alone -> the one of the layers before it. Giving neither output is an error.
 * variant: see "lstm_q8_variant". Synchronises. */
int bh_lstm_q8_layer(const void* x, float bound, const float* w_ih, const float* w_hh, const float* bias, int T, int N, int H,
                     int reverse, int variant, void* h16_out, int8_t* hq_frag, int32_t* sums, void* stream);
/* The same call with the launch split forced. max_rings_per_launch: 0 = as many rings per launch as the device holds (which is
 * bh_lstm_q8_layer); n > 0 = at most n, never more than the device holds, so that the split into several launches runs on a small batch. */
int bh_lstm_q8_layer_split(const void* x, float bound, const float* w_ih, const float* w_hh, const float* bias, int T, int N, int H,
                           int reverse, int variant, void* h16_out, int8_t* hq_frag, int32_t* sums, int max_rings_per_launch,
                           void* stream);

/* The recurrent kernel families of csrc/lstm.hip (BH_LSTM_Q8: csrc/lstm_q8.hip). The widths named below are read off the instance
 * table of lstm.hip (bh_lstm_launch_plan reports it); tests/test_gpu_lstm.py keeps an independent list. */
enum bh_lstm_family {
    BH_LSTM_WAVE = 0,    /* gate GEMM + one wave per 16 units, W_hh in registers: H % 32 == 0, H <= 512 */
    BH_LSTM_FUSED = 1,   /* the same with the input projection inside the recurrence */
    BH_LSTM_STREAM = 2,  /* gate GEMM + W_hh re-read every step: H % 64 == 0, H <= 1024 */
    BH_LSTM_WGX = 3,     /* workgroup-shared, hand-off through a ring buffer: H = 64, 96, 128, 192, 256, 288, 384 */
    BH_LSTM_WGX2 = 4,    /* the same, two rings per workgroup */
    BH_LSTM_CTA = 5,     /* a ring in one workgroup: H = 64, 96, 128 */
    BH_LSTM_WIDE = 6,    /* gate GEMM + stationary W_hh, rings of 32 chunks: H = 640, 768, 896, 1024 */
    BH_LSTM_Q8 = 7       /* the 8-bit path (bh_lstm_q8_layer) */
};
/* Operator level (parity tests): one fp16 recurrent layer on a CHOSEN kernel family, straight from fp32 HOST weights W_ih, W_hh
 * [4H][H] and bias [4H] (b_ih + b_hh, or NULL), packed as bh_encoder_create packs them. x: device fp16 [T][N][H]; h_out: device
 * fp16 [T][N][H], 16-byte aligned. Allocates what the family needs (XCD workspace, the armed ring buffer, the sentinel fill of
 * h_out, the gate tensor of the families that take a GEMM first), launches the family ONCE, synchronises and reads the timeout
 * flag. flags bit 0: the placement-independent write-through exchange; bit 1 (BH_LSTM_WIDE only): the older hand-off through the
 * output tensor, as "lstm_exchange" 0. Errors, never a substitute kernel: a family that has no instance for H, BH_LSTM_Q8, N that
 * is no multiple of the family's ring (16 chunks; 32 for BH_LSTM_WIDE), more rings than one launch holds, an exchange timeout. */
int bh_lstm_layer_family(const void* x, const float* w_ih, const float* w_hh, const float* bias, int T, int N, int H, int reverse,
                         int family, int flags, void* h_out, void* stream);
/* Test hook: the launch the library would make of `n_rings` rings (the whole batch, exchange buffer armed) of family `family` at
 * hidden size H on a device of `cu_count` CUs. Touches no device. flags bits 0-7: the variant - fp16 families: bit 1 as in
 * bh_lstm_layer_family; BH_LSTM_Q8: "lstm_q8_variant" - bits 8 and up: "lstm_tune". Writes BH_LSTM_PLAN_RECORD integers (n_out = room
 * in out):
 *   0 the family has an instance for H, 1 chunks per ring, 2 workgroups per group of 8 slots, 3 rings per slot, 4 workgroups per CU,
 *   5 one workgroup per ring and any number of rings per launch, 6 rings one launch holds on cu_count CUs
 *   7 grid, 8 block, 9 dynamic LDS bytes, 10 the max-dynamic-LDS attribute is raised first
 *   11 bytes of XCD agreement slots armed, 12 bytes of exchange ring buffer armed, 13 exchange-buffer bytes per ring and time slot
 *   (the stride of a split batch), 14-16 the kernel's template key: k-steps, M tiles per wave, flags (fp16: bit 0 = STREAM / RX,
 *   bit 1 = STATS; BH_LSTM_Q8: workgroups per CU)
 * A launch the library refuses is a non-zero return with its message; 0-6 are still written where the family has an instance. */
enum { BH_LSTM_PLAN_RECORD = 17 };
int bh_lstm_launch_plan(int family, int H, int flags, int n_rings, int cu_count, int32_t* out, int n_out);

/* Process-wide knobs (measurement / tuning hooks, no reference counterpart): the rows of the option table in csrc/options.cpp, every
 * one described here (tests/test_abi.py holds the two lists to each other). Not thread-safe: set them while nothing else calls into
 * the library. Values are stored as given unless a row says otherwise; an unknown name is an error.
 *   "beam_fork": -1 auto (default: where the scan is a kernel of its own - up to 64 states, and 1024 states, where the beam kernel
 *                is one wave per chunk), 0 = run the posterior scan behind the beam kernel on the caller's stream,
 *                1 = run it next to the beam kernel on an internal helper stream (joined before finalize).
 *   "beam_fuse": -1 (default) = auto: fused for <= 256 states; 1 = the forward / posterior scan runs as a second wave inside the beam kernel's workgroups and reads
 *                the score and guide rows from the blocks the beam wave stages in LDS (the score tensor is read from HBM once
 *                for both); 0 = separate crf_forward_post_kernel as in round 1 (then "beam_fork" applies).
 *   "beam_cpw": chunks per workgroup of the fused beam kernel at 256 states: 0 (default) = the smallest of 1 / 2 / 4 that lets all
 *                chunks of the call be resident at once (5 / 6 / 8 chunks per CU; the kernels are latency chains, so chunks in
 *                flight per CU are what counts: 2048 x 1667 steps 12.0 -> 8.7 ms on MI355X); 1, 2, 4 force a geometry. Same bytes.
 *   "attn_waves": 0 (default) = automatic, 8 / 12 = waves per workgroup of the ring attention kernel (query blocks of 128 / 192; same results).
 *   "attn_version": 2 (default) = the current ring attention kernel, 1 = the first ring kernel (any other value is stored as 2).
 *   "attn_expt": bit mask of timing experiments of the ring attention kernel, for builds that compile them in. RESULTS ARE WRONG ON
 *                PURPOSE for any value but 0 (the default): each bit removes a part of the kernel to time the rest.
 *   "beam_select": 0 (default) = top-W selection by histogram + exact boundary ranking, 1 = MSB-first radix search
 *                (the same beams either way; kept for regression tests and A/B timing).
 *   "decode_nt": 0 (default) / 1 = the decode kernels read scores and guide rows with the non-temporal cache policy (they are read
 *                once; keeps the L2 for the recurrent kernels when the decoder runs beside the next batch's encoder). Same bytes.
 *   "viterbi_quad": 1 (default) = bh_crf_viterbi on its four-states-per-thread kernel where the layout allows, 0 = the one-state
 *                kernel everywhere. Same bytes.
 *   "conv_ws": 1 (default) = weight-stationary kernel for the 384-channel / 19-tap convolution, 0 = generic implicit GEMM.
 *   "conv_fuse": 1 (default) = conv1 -> conv2 -> conv3 of a 384-channel LSTM stack as one kernel (intermediates in LDS), 2 = also
 *                for the 96-channel stacks, 0 = three kernels. "conv_fs": 1 (default) = feature-split instances of the implicit-GEMM
 *                kernel for layers with a multiple of 64 output channels, 0 = position-split. "conv_lds_kb": LDS a workgroup of that
 *                kernel may take for its input span (default 64; values <= 0 restore it). All of them: identical bytes (tests).
 *   "conv_front_pipe": 1 (default) = the fused front end of a 384-channel stack as a pipeline: 12-wave workgroups, one per CU, each
 *                walking a contiguous run of 256-position blocks; four waves compute conv1 / conv2 of the next block into a second
 *                LDS span buffer while eight waves run conv3 of the current one. 0 = the phase-after-phase kernel (one 8-wave
 *                workgroup per block), which also serves the 96-channel stacks. Identical bytes.
 *   "conv_front_wgs": 0 (default) = one workgroup of the pipelined front end per CU; n > 0 caps the grid at n workgroups, so that a
 *                workgroup walks more blocks (test hook and A/B knob). Identical bytes.
 *   "gemm_path": 0 auto (default), 1 = register-staged 128x128x64 kernel only, 2 = never a 256x256x64 kernel, 3 = never the
 *                four-wave kernel (gemm_w4_kernel; the eight-wave one where it applies), 5 = the four-wave kernel for every legal shape.
 *   "gemm_tile16": 1 (default) = the four-wave kernel's K-tile stream on 16x16x32 MFMAs with its epilogues in the accumulator layout,
 *                0 = the 32x32x16 stream of rounds 4-5 (results agree to fp16 rounding: another accumulation order).
 *                "gemm_order": 1 (default) = an XCD sweeps all feature groups of a block of token tiles before it moves on, 0 = token
 *                blocks fastest; "gemm_gf": feature tiles per block of that order: 0 = automatic, any other value is rounded down to
 *                the nearest of 1 / 2 / 4 / 8 / 16 / 32 and to the number of feature tiles. Same bytes either way. ("gemm_tile16" and
 *                "gemm_order" are stored as 0 / 1.)
 *   "gemm_stagger": 0 (default) = off; n > 0 = the workgroups of an XCD start the persistent 256x256 kernels in eight phase groups,
 *                n x 256 cycles apart in the four-wave kernel, n x ~1024 in the eight-wave one (measured without effect). Same bytes.
 *   "lstm_q8_variant": geometry of the 8-bit recurrent kernel chosen at bh_encoder_create: 0 (default) = 12 / 16 units per wave,
 *                one workgroup per CU; 1 = 4 units per wave, three workgroups per CU; 2 = 12 units per wave compiled for two
 *                workgroups per CU, so that the recurrent kernels of two engines (two batches in flight) share every CU and each
 *                hides the other's exchange round trip (both: hidden size 384 only).
 *   "lstm_max_spins": bound of the recurrent kernels' exchange spin loops (default 1000000; < 0 restores it). Tests lower it
 *                to provoke the timeout path (bh_encoder_error_flag / bh_encoder_check). */
int bh_set_option(const char* name, int value);

/* Posterior decoding = SeqdistModel.decode_batch (crf/model.py:196-199): Viterbi over log(edge posteriors + 1e-8).
 * scores: contiguous koi layout [N][T][4S]; moves/path as bh_crf_viterbi.
 * workspace: bh_crf_posterior_viterbi_workspace(N, T, state_len) bytes. */
size_t bh_crf_posterior_viterbi_workspace(int N, int T, int state_len);
int bh_crf_posterior_viterbi(const void* scores, int N, int T, int state_len, float blank_score, void* workspace,
                             int8_t* moves, int8_t* path, void* stream);

/* Beam-search decode: drop-in for koi.decode.beam_search(scores, beam_width=32, beam_cut=100.0, scale=1.0,
 * offset=0.0, blank_score=2.0) (bonito/crf/basecall.py:27,36-40).  scores: device fp16 contiguous
 * [N][T][4^(state_len+1)] (koi layout).  Outputs are DEVICE int8 [N][T], zero where nothing is emitted:
 * sequence = ASCII base at emitting steps, qstring = 33 + round(q), moves in {0,1}; qfloat (optional,
 * device fp32 [N][T]) receives the un-rounded q.  workspace: bh_beam_search_workspace(N, T, state_len) bytes.
 * Algorithm "BS-2" (round 5: the guide and the posterior scan in the linear domain, a deterministic exponential shared with the oracle;
 * DESIGN.md 5); bit-exact against oracle/crf_oracle.c for sequence and moves, q within 1e-3 of its fp64 posteriors.
 * Limits: 1 <= state_len <= 5, 1 <= beam_width <= 32, beam_cut >= 1, T < 131072 steps per chunk. */
size_t bh_beam_search_workspace(int N, int T, int state_len);
int bh_beam_search(const void* scores, int N, int T, int state_len, int beam_width, float beam_cut,
                   float blank_score, float q_scale, float q_offset, void* workspace, int8_t* sequence,
                   int8_t* qstring, int8_t* moves, float* qfloat, void* stream);
/* TEST HOOK: what bh_beam_search would launch, and bh_beam_search / bh_crf_logz / bh_crf_posterior_viterbi carve out of their
 * workspace, for (N, T, state_len) under the current bh_set_option values, on a device of cu_count compute units, with (debug != 0)
 * or without the BH_BEAM_DEBUG counters. Touches no device. Writes BH_BEAM_PLAN_RECORD integers (n_out = room in out):
 *   0..3    backward scan of the beam search: state_len of the instance, grid, block, dynamic LDS bytes
 *   4..9    forward / posterior scan as a kernel of its own: present, state_len, grid, block, LDS bytes, asked onto the helper stream
 *           (all 0 where the scan is a wave of the beam kernel)
 *   10..16  beam kernel: its template arguments state_len, chunks per workgroup, debug, fused; grid, block, LDS bytes
 *   17, 18  selection by radix search ("beam_select"), non-temporal staging ("decode_nt")
 *   19..38  the workspace layout, each value as (low, high) 32-bit halves: byte offsets of beta~, Bcum, logZ, P, the beam back-pointers,
 *           the final slots, the debug counters and the posterior-Viterbi back-pointer plane, then bh_beam_search_workspace and
 *           bh_crf_posterior_viterbi_workspace. */
enum { BH_BEAM_PLAN_RECORD = 39 };
int bh_beam_search_plan(int N, int T, int state_len, int cu_count, int debug, int32_t* out, int n_out);

/* ---- operator level (parity tests, custom pipelines) ----------------------------------------- */
/* out[m][n] = clamp(act(X[m][:] . W[n][:] + bias[n]) * scale); fp16 X [M][ldx], W [N][ldw], out [.][ldo].
 * gated=1: SwiGLU epilogue over interleaved rows (out has N/2 columns).
 * row remap: out_row = (m / row_div) * row_s_hi + (m % row_div) * row_s_lo   (row_div=0: identity);
 * rows with (m % row_div) >= row_lim are skipped (row_lim=0: none) -- used to drop batch padding. */
int bh_linear(const void* X, const void* W, const float* bias, void* out, int M, int N, int K, int ldx,
              int ldw, int ldo, int act, float scale, float clamp_lo, float clamp_hi, int gated,
              int row_div, long row_s_hi, long row_s_lo, int row_lim, void* stream);
/* bh_linear with the fused residual the transformer's out_proj / fc2 and the residual convolution branches use. Order of the epilogue,
 * all in fp32 with ONE rounding to fp16 at the end:  z = X[m] . W[n] + bias[n];  z += res_scale * residual[m][n]  (the residual is indexed
 * by the INPUT row m, not by the remapped output row; fp16 [M][ldres]);  activation;  * scale;  clamp.  With gated=1 the residual
 * (N columns) is added to the interleaved (y, gate) pairs BEFORE gating, and scale / clamp apply to y * swish(gate).
 * ldres must be a multiple of 8 halves like ldx / ldw / ldo (the kernels read the residual in 16-byte vectors): anything else is an
 * error (nonzero return, nothing launched). */
int bh_linear_residual(const void* X, const void* W, const float* bias, void* out, int M, int N, int K, int ldx,
                       int ldw, int ldo, int act, float scale, float clamp_lo, float clamp_hi, int gated,
                       int row_div, long row_s_hi, long row_s_lo, int row_lim, const void* residual, int ldres,
                       float res_scale, void* stream);
/* Packed Wqkv projection with the rotary embedding fused into its epilogue (what the engine's transformer layers run):
 * X fp16 [M][K], W fp16 [3D][K], bias fp32 [3D] or null, out fp16 [M][3D]; D % 64 == 0 (heads of 64), K % 8 == 0. Row m has position
 * m % T; cos_sin = device copy of bh_rotary_table(>= T, 64). Per head of 64 (x1 = dims 0..31, x2 = dims 32..63, non-interleaved):
 * out[0:D) = (x1 cos - x2 sin, x1 sin + x2 cos) of q, times qscale; out[D:2D) = the same rotation of k; out[2D:3D) = v unchanged. */
int bh_linear_qkv_rotary(const void* X, const void* W, const float* bias, void* out, int M, int D, int K,
                         const float* cos_sin, int T, float qscale, void* stream);
/* TEST HOOK: the kernel the last bh_linear* call (or linear layer of an encoder) of this process launched: 1 = register-staged 128-tile
 * kernel, 2 = LDS-DMA 128-tile kernel, 3 = eight-wave 256-tile kernel, 5 / 6 = four-wave 256-tile kernel on its 32x32x16 / 16x16x32
 * stream; 0 = none yet. A host-side static written by the launcher: process-wide, not thread-safe. */
int bh_linear_last_kernel(void);
/* first convolution, Cin = 1: signal fp16 [N][Lin] -> out (n*os_n + t*os_t + c), w fp32 [Cout][K] on device */
int bh_conv1d_first(const void* signal, const float* w, const float* bias, void* out, int N, int Lin,
                    int Cout, int K, int stride, int pad, int act, float clamp_lo, float clamp_hi,
                    long os_n, long os_t, void* stream);
/* packed conv weight size in halves and host-side packer: torch [Cout][Cin][K] fp32 -> [Cout16][Kp] fp16 */
size_t bh_conv1d_packed_halves(int Cin, int Cout, int K);
int bh_conv1d_pack(const float* w, int Cin, int Cout, int K, uint16_t* packed);
/* channel-minor implicit-GEMM conv: in fp16 [N][Lin][Cin] -> out (n*os_n + t*os_t + c). Cin % 8 == 0, Cout % 4 == 0, os_n and os_t
 * multiples of 4. The weight-stationary kernel (384 / 96 channels, ten k-steps) is taken only with a null or 16-byte aligned bias. */
int bh_conv1d(const void* in, const void* wpacked, const float* bias, void* out, int N, int Lin, int Cin,
              int Cout, int K, int stride, int pad, int act, float clamp_lo, float clamp_hi, long os_n,
              long os_t, void* stream);
/* The fused front end of an LSTM model: conv1 (1 -> 16 channels, K1 taps, stride 1) -> conv2 (16 -> 16, K2 taps, stride 1) -> conv3
 * (16 -> Cout3 channels, K3 taps, stride3) in one kernel, the 16-channel intermediates never leaving the CU; each layer with its own
 * padding, activation and clamp, each computed by the operations of bh_conv1d_first / bh_conv1d / bh_conv1d in their order (identical
 * bytes). signal fp16 [N][L0]; w1 fp32 [16][K1], b1 / b2 / b3 fp32 or null (b3 16-byte aligned); w2packed = bh_conv1d_pack(16, 16, K2),
 * w3packed = bh_conv1d_pack(16, Cout3, K3); out (n*os_n + t*os_t + c), os_n and os_t multiples of 4.
 * Shapes with an instance: 1 <= K1 <= 8, K2 <= 6, Cout3 384 or 96, K3 19 or 20 (ten k-steps of 32), stride3 small enough for the
 * workgroup's LDS (<= 7 at these sizes). Anything else is an error (nonzero return, nothing launched, output untouched). The process-wide
 * options "conv_fuse" / "conv_ws" decide what the ENGINE runs; this entry point does not read them. It reads "conv_front_pipe" and
 * "conv_front_wgs", which pick between the two 384-channel instances and size the pipelined one's grid (identical bytes). */
int bh_conv1d_front3(const void* signal, int N, int L0, const float* w1, const float* b1, int K1, int pad1, int act1, float lo1,
                     float hi1, const void* w2packed, const float* b2, int K2, int pad2, int act2, float lo2, float hi2,
                     const void* w3packed, const float* b3, int Cout3, int K3, int stride3, int pad3, int act3, float lo3,
                     float hi3, void* out, long os_n, long os_t, void* stream);
/* TEST HOOK: the kernel and instance the last convolution launch of this process took (bh_conv1d_first, bh_conv1d, bh_conv1d_front3,
 * bh_dwconv1d, or a convolution layer of an encoder), as one of the codes below; 0 = none yet. A host-side static written by the
 * launchers: process-wide, NOT thread-safe. */
enum bh_conv_kernel {
    BH_CONV_K_NONE = 0,
    BH_CONV_K_FIRST = 1,          /* conv_first_kernel */
    BH_CONV_K_WS_384 = 20,        /* conv_ws_kernel<3, 10, 8>: weight-stationary, 384 channels */
    BH_CONV_K_WS_96 = 21,         /* conv_ws_kernel<1, 10, 6>: 96 channels */
    BH_CONV_K_FRONT3_384 = 30,    /* conv_front3_kernel<3, 10, 8>, or conv_front3_pipe_kernel<3, 10> under "conv_front_pipe" */
    BH_CONV_K_FRONT3_96 = 31,     /* conv_front3_kernel<1, 10, 6> */
    BH_CONV_K_DWCONV = 40,        /* dwconv_kernel */
    BH_CONV_K_IGEMM_BASE = 100    /* conv_igemm_kernel<NTT, FS>: 100 + 10 * NTT + FS, NTT in 1 / 2 / 4 (64 / 128 / 256 positions per workgroup) */
};
#define BH_CONV_K_IGEMM(ntt, fs) (BH_CONV_K_IGEMM_BASE + 10 * (ntt) + (fs))
int bh_conv1d_last_kernel(void);
/* Greedy CTC decode of R reads in one launch: replaces fast_ctc_decode.viterbi_search(probs, alphabet,
 * qstring=True, qscale, qbias) (bonito/ctc/model.py:39-42).  logp: device fp32 [sum T_r][classes]
 * log-probabilities, offsets: device int64 [R+1].  Outputs (device, compacted per read at offsets[r]):
 * labels (1..classes-1), qual (phred chars), path (step of each base), count[R]. */
int bh_ctc_greedy_decode(const float* logp, const long* offsets, int R, int classes, float qscale, float qbias,
                         int8_t* labels, int8_t* qual, int* path, int* count, void* stream);
/* CTC prefix beam search of R reads in one launch: replaces fast_ctc_decode.beam_search(probs, alphabet, beam_size=5,
 * beam_cut_threshold=1e-3) (bonito/ctc/model.py:44).  Same buffers as bh_ctc_greedy_decode (no qualities);
 * workspace: bh_ctc_beam_search_workspace(sum T_r, R, classes, beam_size) device bytes. beam_size <= 16. */
size_t bh_ctc_beam_search_workspace(long total_steps, int R, int classes, int beam_size);
int bh_ctc_beam_search(const float* logp, const long* offsets, int R, int classes, int beam_size, float threshold,
                       void* workspace, int8_t* labels, int* path, int* count, void* stream);
/* depthwise conv (TCSConv1d.depthwise, ctc/model.py:99-103): in/out fp16 channel-minor [N][L][C], w fp32 device [C][K] */
int bh_dwconv1d(const void* in, const float* w, void* out, int N, int Lin, int C, int K, int stride, int pad,
                void* stream);
/* CTC head (Decoder, ctc/model.py:195-207): the 1x1 decoder convolution and log_softmax over the classes in one kernel.
 * in fp16 [M][features], w fp32 device [classes][features], bias fp32 device [classes] -> out fp16 [M][classes] log-probabilities
 * (fp32 logits and softmax, one rounding at the store). 1 <= classes <= 8, features a positive multiple of 8, and the weights
 * (classes * features * 4 bytes) must fit 64 KiB of LDS; anything else is refused on the host. */
int bh_ctc_head(const void* in, const float* w, const float* bias, void* out, long M, int features, int classes,
                void* stream);
/* rotary cos/sin table (host): out[t][i][0..1] = cos, sin(t * 10000^(-2i/dim)), i < dim/2, fp32
 * (flash_attn.layers.rotary.RotaryEmbedding(dim, interleaved=False), bonito/transformer/model.py:55,73) */
int bh_rotary_table(int T, int dim, float* out);
/* rotary + sliding-window attention on packed qkv (flash_attn_qkvpacked_func(qkv, window_size=(l, r)),
 * bonito/transformer/model.py:58-66): qkv fp16 [N*T][3*nhead*head_dim] -> out fp16 [N*T][nhead*head_dim];
 * cos_sin = device copy of bh_rotary_table(T, head_dim). head_dim must be 64. */
int bh_attention(const void* qkv, void* out, const float* cos_sin, int N, int T, int nhead, int head_dim,
                 int win_left, int win_right, void* stream);
/* The same windowed attention on packed qkv whose q and k ALREADY carry the rotary embedding and whose q is scaled by log2(e) / sqrt(head_dim)
 * (what the engine's Wqkv epilogue writes): the persistent ring-buffer kernel the engine runs for windows with left <= 128 and
 * right <= 144 (flash_attn_qkvpacked_func proper, bonito/transformer/model.py:60; softmax in base 2 on pre-scaled scores). Any other
 * window is an error (nonzero return, output untouched): such a layer is served by bh_attention, in the engine too. */
int bh_attention_prerotated(const void* qkv, void* out, int N, int T, int nhead, int head_dim, int win_left, int win_right, void* stream);
/* out = rmsnorm(a + alpha * x) * w (fp32 statistics, eps inside the root): RMSNorm(x, residual) of bonito/transformer/model.py:110-111,125-128.
 * a, x, out fp16 [M][D], w fp32 device [D]; D a multiple of 8, 8 <= D <= 1024. x == NULL means that `a` already holds the residual sum
 * (the engine can fuse alpha * x into the epilogue of the producing GEMM); alpha is then not read. `out` must not alias `a` or `x`:
 * the engine never calls it in place, and in-place is not a supported call. */
int bh_rmsnorm_residual(const void* a, const void* x, const float* w, void* out, long M, int D, float alpha,
                        float eps, void* stream);
/* recurrent weights: torch W_hh [4H][H] fp32 (host) -> MFMA-fragment order fp16 (host, 4*H*H halves) */
int bh_lstm_pack_whh(const float* whh, int H, uint16_t* packed);
/* host helper of the formatting stage = koi.decode.to_str before the text decode (bonito/crf/basecall.py:48-55): copies the
 * non-zero bytes of src[0..n) to dst (capacity n) in order and returns how many there were. No device work. */
long bh_host_compact(const int8_t* src, long n, char* dst);
/* host helper of the chunking stage: rows [row0, row0 + nrows) of util.chunk(signal[0..T), chunksize, overlap)
 * (bonito/util.py:142-161; T >= chunksize) cast to fp16 (round to nearest even) into dst[nrows][chunksize].
 * Returns nrows, or < 0 on bad arguments. No device work. */
long bh_host_chunk_rows(const float* signal, long T, int chunksize, int overlap, long row0, long nrows, uint16_t* dst);

/* One basecalled read -> its FASTQ (mode 0) / FASTA (1) / unaligned SAM (2) record, in one call: the stitching of
 * bonito/util.py:164-183 (via crf/basecall.py:13-24: the kept window of every chunk, `reverse` included), koi's to_str
 * (crf/basecall.py:48-55), the rna flip, the mean q-score filter and the record text with the tags of bonito/io.py:135-166
 * (RG:Z, qs:f, ns:i, ts:i, mv:B:c). The read's chunks are n_pieces runs of consecutive rows of decoded planes: piece i = rows
 * [lo[i], lo[i] + rows[i]) of an int8 array [3][n][T] (sequence, qstring, moves) at base[i] whose planes are plane_stride[i] bytes
 * apart. Returns the bytes written to out; 0 = filtered out (empty sequence or mean q < min_qscore; seq_len / mean_q are set
 * regardless); -1 = bad arguments; < -1 = -(bytes of out needed). */
long bh_host_format_read(const int8_t* const* base, const long* plane_stride, const long* lo, const long* rows, int n_pieces,
                         long T, long length, int chunksize, int overlap, int stride, int reverse, int rna, int mode,
                         double min_qscore, const char* read_id, const char* run_id, long num_samples, long trimmed_samples,
                         char* out, long out_cap, long* seq_len, double* mean_q);
/* Host only. One mapped read of the mapper (bh_map_*; bonito_amd/aligner.py): runs = the run words of bh_nw_align for its pieces, in
 * order ((length << 2) | op, ops = X I D = 0 1 2 3), walked over the read's codes q (on the aligned strand) from q_st and the contig's
 * codes r from r_st (1..4 = A C G T, anything else = no base) -> cigar: the run words of the M I D CIGAR ((length << 2) | 0 1 2; = and
 * X are M, equal neighbours merged), cigar_text: the same as text (not terminated), md: the MD string (not terminated; a column matches
 * when both codes are the same base; other reference codes print as N). counts (int64 [8]): NM, matching columns, all columns, CIGAR
 * runs, bytes of cigar_text, bytes of md, the query and the reference position behind the last column. Returns 0; -1 = bad
 * arguments or runs that leave a sequence; -3 = cigar_cap (runs), cigar_text_cap or md_cap (bytes) too small: n_runs runs,
 * 24 bytes per run and 24 bytes per run plus 2 per column always suffice. */
long bh_host_map_finish(const uint32_t* runs, long n_runs, const int8_t* q, long q_len, long q_st, const int8_t* r, long r_len, long r_st,
                        uint32_t* cigar, long cigar_cap, char* cigar_text, long cigar_text_cap, char* md, long md_cap, int64_t* counts);
/* Mean q-score of a phred string, averaged in error-probability space (bonito/util.py mean_qscore_from_qstring). */
double bh_host_mean_qscore(const char* qstring, long n);
/* pod5 signal codec, inner layer (bonito_amd/pod5.py; replaces the pod5 wheel behind /root/reference bonito/pod5.py:52 `read.signal`):
 * streamvbyte-16 over the zig-zag code of the first differences -> `count` int16 samples. `in` is the zstd-DEcompressed block.
 * Returns the bytes consumed, -1 when the input is too short. Host code, no device involved. */
long bh_host_svb16_decode(const uint8_t* in, long n_in, long count, int16_t* out);
/* one LSTM layer over gates_in = x W_ih^T + b (fp16 [T][N][4H], torch gate order); h_out fp16 [T][N][H].
 * N % 16 == 0.  workspace: bh_lstm_workspace(N, H) device bytes.  err_flag: device int, set non-zero on a
 * device-side timeout.  flags bit 0: force the placement-independent write-through exchange policy;
 * bit 1: force the weight-streaming kernel (always used for H > 512; needs H % 64 == 0, H <= 1024). */
size_t bh_lstm_workspace(int N, int H);
int bh_lstm_layer(const void* gates_in, const void* whh_packed, void* h_out, int T, int N, int H,
                  int reverse, void* workspace, int* err_flag, int flags, void* stream);

/* ---- the optimizer step behind backward(): unscale, gradient norm, overflow check, clip, AdamW, loss scale (csrc/optim.hip) ----------
 * Per tensor i of n[i] elements: p, m, v (fp32, updated in place) and g (fp32, never written), DEVICE pointers in HOST arrays; they
 * travel to the kernels by value, at most 32 tensors per launch, so there is no per-step copy and no table in device memory.
 * ctl: DEVICE double [BH_OPTIM_CTL_WORDS], the control block. The caller initialises SCALE (the loss scale), GROWTH_TRACKER = 0,
 *   STEP = 0, BETA1_POW = BETA2_POW = 1; the other words are written by every bh_optim_norm call.
 * bh_optim_norm (once per step, over every tensor of every parameter group):
 *   partial sums: one workgroup of 256 threads per chunk of BH_OPTIM_CHUNK elements writes the fp32 sum of g^2 of its chunk to slot
 *     (launch, workgroup) of the workspace; the split and the order of the additions depend on the sizes alone.
 *   finalise, one wave: sum = the slots added in fp64 (lane l the slots l, l + 64, ..; then the lanes in order);
 *     scale = use_scale ? ctl[SCALE] : 1;  GRAD_NORM = sqrt(sum) / scale;  SKIPPED = !isfinite(sum);  SCALE_USED = scale;
 *     not skipped: STEP += 1, BETA1_POW *= beta1, BETA2_POW *= beta2, CLIP_COEF = max_norm > 0 ? min(1, max_norm / (GRAD_NORM + 1e-6)) : 1,
 *       GRAD_MUL = CLIP_COEF / scale, BIAS1 = 1 - BETA1_POW, BIAS2_SQRT = sqrt(1 - BETA2_POW);   skipped: CLIP_COEF = GRAD_MUL = 0;
 *     use_scale (torch's GradScaler): skipped -> SCALE *= backoff, GROWTH_TRACKER = 0; otherwise ++GROWTH_TRACKER == growth_interval
 *       -> SCALE *= growth, GROWTH_TRACKER = 0.
 * bh_optim_update (once per parameter group, behind bh_optim_norm on the same stream), elementwise and operation by operation in fp32,
 *   the scalars rounded to fp32 once:  gs = g * (float)GRAD_MUL;  p = p * (float)(1 - lr * weight_decay);  m = beta1 * m + (1 - beta1) * gs;
 *   v = beta2 * v + ((1 - beta2) * gs) * gs;  denom = sqrt(v) / (float)BIAS2_SQRT + eps;  p = p - (float)(lr / BIAS1) * (m / denom),
 *   divide and square root correctly rounded. With SKIPPED set the kernel returns in front of its first store.
 *   float4 accesses where p, g, m and v of a tensor are all 16-byte aligned, scalar ones otherwise (same arithmetic).
 * workspace: bh_optim_workspace(n, n_tensors) bytes (0 = bad sizes), the caller's, 4-byte aligned.
 * Bad arguments (null pointers, n < 1, lr / eps / weight_decay / betas out of range, a small workspace) return nonzero with
 * bh_last_error() set and launch nothing. Stream-ordered; nothing is allocated and nothing synchronises inside.
 * TEST HOOK bh_optim_last_kernel: the access paths the last bh_optim_update of this thread used, BH_OPTIM_K_VECTOR | BH_OPTIM_K_SCALAR. */
#define BH_OPTIM_CHUNK 8192
enum bh_optim_ctl {
    BH_OPTIM_SCALE = 0, BH_OPTIM_GROWTH_TRACKER = 1, BH_OPTIM_STEP = 2, BH_OPTIM_BETA1_POW = 3, BH_OPTIM_BETA2_POW = 4,
    BH_OPTIM_GRAD_NORM = 5, BH_OPTIM_CLIP_COEF = 6, BH_OPTIM_SKIPPED = 7, BH_OPTIM_SCALE_USED = 8, BH_OPTIM_GRAD_MUL = 9,
    BH_OPTIM_BIAS1 = 10, BH_OPTIM_BIAS2_SQRT = 11, BH_OPTIM_CTL_WORDS = 16
};
enum bh_optim_kernel { BH_OPTIM_K_VECTOR = 1, BH_OPTIM_K_SCALAR = 2 };
int bh_optim_chunk(void);
size_t bh_optim_workspace(const long* n, int n_tensors);
int bh_optim_norm(const float* const* g, const long* n, int n_tensors, double* ctl, double max_norm, int use_scale, double growth,
                  double backoff, int growth_interval, double beta1, double beta2, void* workspace, size_t workspace_bytes, void* stream);
int bh_optim_update(float* const* p, const float* const* g, float* const* m, float* const* v, const long* n, int n_tensors,
                    const double* ctl, double lr, double beta1, double beta2, double eps, double weight_decay, void* stream);
int bh_optim_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif /* BONITO_HIP_H */
