// Host side of libbonito_hip.so: error plumbing and the encoder engine (a linear chain of layers executed as
// hand-written HIP kernels on one stream) behind the bh_encoder_* functions of include/bonito_hip.h. The
// operator-level shells are in abi.cpp.
//
// The engine is the MI355X replacement for what the reference obtains from
// koi.lstm.update_graph + cuDNN/cuBLAS under SeqdistModel.forward
// (the reference's bonito/crf/model.py:193-194,240-246): it owns fp16 copies of the weights,
// all activation workspace (sized once for max_batch x max_chunk; HBM is 288 GB so nothing is
// re-allocated per batch) and runs conv -> [permute folded] -> LSTM x L -> LinearCRFEncoder
// [-> clamp folded] writing NTC fp16 scores straight into the caller's buffer.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/bonito_hip.h"
#include "common.h"
#include "devbuf.h"
#include "kernels.h"
#include "lstm_pack.h"
#include "options.h"

// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
void bh_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* bh_last_error(void) { return g_err; }
extern "C" int bh_abi_version(void) { return BH_ABI_VERSION; }
extern "C" size_t bh_sizeof_layer(void) { return sizeof(bh_layer_t); }
extern "C" int bh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        bh_set_error("hipGetDeviceCount failed");
        return -1;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------
namespace {

struct Layer {
    bh_layer_t d;        // descriptor (host pointers are not kept)
    DevBuf w0, w1, w2, w3, w4, w5, b0, b1;
    bool fused_clamp = false;   // a following CLAMP was folded into this layer
    float clamp_lo = -INFINITY, clamp_hi = INFINITY;      // (the identity unless fused_clamp)
    // convolution: channel counts as laid out in memory. Channel-minor activations between two
    // convolutions are padded to a multiple of 8 channels (zero weights / zero bias -> act(0) = 0),
    // so e.g. the old-style 1 -> 4 -> 16 front end (crf/model.py:153-154) still runs on MFMA.
    int cin_eff = 0, cout_eff = 0;
    bool pointwise = false;     // K=1, stride 1 convolution executed by the GEMM kernel (supports the residual add)
    // 8-bit recurrent path (Q8-1, lstm_q8.hip): int8 weight tiles, per-row scales (s_ih * bound/127, s_hh/127), bound of the input
    bool q8 = false;
    bool q8_only = false;       // no fp16 family has an instance for this width (144, 336): the "lstm_q8" A/B switch cannot turn it off
    int q_variant = 0;
    float q_bound = 1.0f;
    DevBuf q_wih, q_whh, q_sx, q_sh;
    // recurrent layer, fp16: W_ih and W_hh in every layout that a kernel family the shape admits wants (kernels.h: bh_lstm_layout;
    // the tiles are of 4 * lstm_mt units). b0 is b_ih + b_hh in torch order, lstm_bias_wide the same for the wide kernel's gate GEMM.
    DevBuf lstm_ih[BH_LSTM_W_LAYOUTS], lstm_hh[BH_LSTM_W_LAYOUTS], lstm_bias_wide;
    int lstm_mt = 0;
};

enum Layout { L_SIGNAL, L_NLC, L_TNC };

// RAII span: records a pair of events around a group of launches when profiling is on.
struct ProfSpan {
    bh_encoder* e; hipStream_t st; int cls; hipEvent_t a = nullptr, b = nullptr;
    ProfSpan(bh_encoder* e_, hipStream_t st_, int cls_);
    ~ProfSpan();
};

static inline int pad8(int n) { return (n + 7) / 8 * 8; }

}  // namespace

// ---- launch helpers shared by the kernel files (declared in common.h) ------------------------------------------------------------------
#include <mutex>
#include <unordered_map>
hipError_t bh_max_lds(const void* fn, int bytes) {
    static std::mutex mu;
    static std::unordered_map<unsigned long long, int> raised;       // (function, device) -> bytes granted so far
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long key = (unsigned long long)(uintptr_t)fn * 64ull + (unsigned)dev % 64u;
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = raised.find(key);
        if (it != raised.end() && it->second >= bytes) return hipSuccess;
    }
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> g(mu);
        int& have = raised[key];
        if (have < bytes) have = bytes;
    }
    return e;
}
int bh_cu_count() {
    static std::atomic<int> cached[64];
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    cus = cached[dev].load(std::memory_order_relaxed);
    if (cus > 0) return cus;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
    cached[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

struct bh_encoder {
    int device = 0;
    int max_batch = 0, max_chunk = 0;
    int n_cus = 0;
    std::vector<Layer> layers;
    DevBuf act[3], gates, sig, err, lstm_ws;
    // Timeout flags are PER FORWARD: forward number n (its "ticket") owns slot n % ERR_SLOTS of `err`; the slot is zeroed on the
    // stream in front of the forward, the persistent recurrent kernels raise it, and a 4-byte copy behind the forward mirrors it
    // into the same slot of the pinned host array. A caller that has observed the completion of forward n reads ITS flag
    // (bh_encoder_error_flag_at) - flags of other forwards in flight are neither consumed nor cleared (advisor finding, round 3:
    // the one sticky flag made a retry of batch i erase the evidence against batches i+1, i+2). At most ERR_SLOTS forwards of an
    // engine may be in flight. `sticky` collects the slots as they are recycled, for bh_encoder_check / bh_encoder_error_flag
    // ("has anything timed out since the last check").
    static constexpr int ERR_SLOTS = 64;
    int* err_host = nullptr;     // pinned [ERR_SLOTS] mirror of `err`
    // (atomics: bh_encoder_forward runs on the encoder thread of the product pipeline while bh_encoder_error_flag_at / _ack / _error_flag
    //  run on its decode thread - ctypes releases the GIL; advisor finding, round 4)
    std::atomic<long> ticket{-1};    // number of the most recent forward
    std::atomic<long> checked{-1};   // forwards <= checked have been reported by bh_encoder_check
    std::atomic<int> sticky{0};      // flags harvested from recycled slots (forwards in (checked, ticket - ERR_SLOTS])
    int* cur_err = nullptr;      // device slot of the forward being issued
    int n_act = 2;               // activation buffers in rotation: 3 when recurrent layers pre-fill their exchange sentinel
    // sentinel pre-fill of the NEXT recurrent layer's output buffer, on a side stream under the current layer's kernel
    hipStream_t fill_stream = nullptr;
    hipEvent_t fill_ready = nullptr, fill_done = nullptr;
    void* prefilled = nullptr;
    int lstm_prefill = 1;
    DevBuf q_act[2], q_ex;                 // 8-bit recurrent path: int8 activations in fragment order, exchange ring buffer
    DevBuf ex16;                           // fp16 workgroup-shared kernel: exchange ring buffer (lstm_layer_wgx_kernel)
    int lstm_pair = 1;                     // batches of more rings than one launch holds: two rings per workgroup instead of two launches
    int norm_fuse = 0;                     // transformer: 1 = alpha * residual added in the out_proj / fc2 epilogues instead of the norm kernel (measured: no gain, 67.7 vs 67.4 ms per sup step - the residual read costs the GEMM epilogue what it saves the norm kernel)
    int lstm_exchange = 1;                 // 1: hand-off through the ring buffer (no sentinel fill of the output tensor), 0: through the output
    int lstm_q8 = 1;                       // 0: run quantised layers through the fp16 kernels (A/B)
    DevBuf res;                            // pending residual projection of a QuartzNet block
    DevBuf t_qkv, t_mid, t_a, t_b, rot;   // transformer workspace + rotary cos/sin table [Tmax][32][2]
    int rot_len = 0;
    int out_features = 0;
    int lstm_force_slow = 0, lstm_tune = 0;
    int batch_pad = 16;          // chunks per LSTM ring: 16, or 32 when a wide (H > 512) layer uses two column tiles per ring
    int lstm_wide = 1;           // H > 512: stationary-W_hh kernel with 32-chunk rings (0: weight-streaming kernel)
    int attn_ring = 1;           // transformer: rotary in the Wqkv epilogue + persistent ring-buffer attention kernel
    int lstm_fused = 3;          // insize == hidden: 3 = + ring-in-a-workgroup kernel for narrow layers, 2 = workgroup-shared fused
                                 // kernel where it covers H, 1 = per-wave fused
                                 // kernel (input projection inside the recurrence), 0 = projection by a GEMM beforehand
    // optional per-kernel-class timing with HIP events on the caller's stream (bench.py roofline leg)
    bool profiling = false;
    struct Span { int cls; hipEvent_t a, b; };
    std::vector<Span> spans;
    ~bh_encoder() {
        for (auto& s : spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
        if (fill_ready) (void)hipEventDestroy(fill_ready);
        if (fill_done) (void)hipEventDestroy(fill_done);
        if (fill_stream) (void)hipStreamDestroy(fill_stream);
        if (err_host) (void)hipHostFree(err_host);
        // (the device buffers free themselves: bh_encoder_destroy makes the engine's device current around the delete)
    }
};

namespace {

ProfSpan::ProfSpan(bh_encoder* e_, hipStream_t st_, int cls_) : e(e_), st(st_), cls(cls_) {
    if (!e->profiling) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
    (void)hipEventRecord(a, st);
}
ProfSpan::~ProfSpan() {
    if (!a) return;
    (void)hipEventRecord(b, st);
    e->spans.push_back({cls, a, b});
}

// Walk the chain for chunks of L samples and batch N (padded): output length and features, the largest activation / gate
// buffer, and the transformer workspace (per-layer maxima over the token count each transformer layer sees).
struct Walk {
    int T = 0, C = 0;
    size_t act_bytes = 0, gate_bytes = 0;
    size_t qkv_bytes = 0, mid_bytes = 0, model_bytes = 0;
    int max_tokens = 0;
};
static int walk(const bh_encoder* e, int N, int L, Walk* w) {
    long len = L;
    int C = 1;
    size_t amax = 0;
    for (const auto& l : e->layers) {
        switch (l.d.kind) {
            case BH_LAYER_CONV:
                len = conv_out_len((int)len, l.d.winlen, l.d.stride, l.d.padding);
                BH_REQUIRE(len > 0, "encoder: chunk of %d samples is too short for the convolution stack", L);
                C = l.d.out_size;
                amax = std::max(amax, (size_t)N * len * std::max(l.cout_eff, C) * 2);
                break;
            case BH_LAYER_LSTM:
                C = l.d.out_size;
                amax = std::max(amax, (size_t)N * len * C * 2);
                w->gate_bytes = std::max(w->gate_bytes, (size_t)N * len * 4 * C * 2);
                break;
            case BH_LAYER_LINEAR_CRF:
                C = l.d.out_size;
                break;
            case BH_LAYER_LINEAR:
                C = l.d.out_size;
                amax = std::max(amax, (size_t)N * len * C * 2);
                break;
            case BH_LAYER_CLAMP:
                break;
            case BH_LAYER_TRANSFORMER: {
                const size_t M = (size_t)N * len;
                amax = std::max(amax, M * C * 2);
                w->qkv_bytes = std::max(w->qkv_bytes, M * 3 * l.d.in_size * 2);
                w->mid_bytes = std::max(w->mid_bytes, M * l.d.dim_ff * 2);
                w->model_bytes = std::max(w->model_bytes, M * l.d.in_size * 2);
                w->max_tokens = std::max(w->max_tokens, (int)len);
                break;
            }
            case BH_LAYER_DWCONV:
                len = conv_out_len((int)len, l.d.winlen, l.d.stride, l.d.padding);
                BH_REQUIRE(len > 0, "encoder: chunk of %d samples is too short for the convolution stack", L);
                amax = std::max(amax, (size_t)N * len * C * 2);
                break;
            case BH_LAYER_RESIDUAL_PROJ:
                amax = std::max(amax, (size_t)N * len * l.d.out_size * 2);   // res buffer uses the same bound
                break;
            case BH_LAYER_CTC_DECODER:
                C = l.d.out_size;
                break;
            case BH_LAYER_UPSAMPLE:
                len *= l.d.scale_factor;
                amax = std::max(amax, (size_t)N * len * C * 2);
                break;
            default:
                BH_REQUIRE(false, "encoder: layer kind %d is not supported by this build", l.d.kind);
        }
    }
    w->T = (int)len;
    w->C = C;
    w->act_bytes = amax;
    return 0;
}

// The layer that consumes layer i's output: clamp layers are folded into their producer and skipped. layers.size() if none.
static size_t next_layer(const bh_encoder* e, size_t i) {
    size_t j = i + 1;
    while (j < e->layers.size() && e->layers[j].d.kind == BH_LAYER_CLAMP) ++j;
    return j;
}
static int next_kind(const bh_encoder* e, size_t i) {
    const size_t j = next_layer(e, i);
    return j < e->layers.size() ? e->layers[j].d.kind : 0;
}

// ---- which recurrent kernel serves a layer (the instance table of lstm.hip) -----------------------------------------------------------
// What a layer's shape admits: the fp16 families that have an instance for its width and, where the input projection is inside the
// kernel, whose input is as wide. bh_encoder_create packs and allocates by these rows, lstm_plan dispatches among them by the
// engine's options: the two cannot disagree.
static const bh_lstm_instance* lstm_admits(const bh_layer_t& d, int family, int variant = 0) {
    const bh_lstm_instance* row = bh_k_lstm_find(family, d.out_size, variant);
    return row && (!row->projects || d.in_size == d.out_size) ? row : nullptr;
}
static std::vector<const bh_lstm_instance*> lstm_admitted(const bh_layer_t& d) {
    std::vector<const bh_lstm_instance*> rows;
    for (int f = BH_LSTM_WAVE; f < BH_LSTM_Q8; ++f)
        if (const bh_lstm_instance* row = lstm_admits(d, f)) rows.push_back(row);
    return rows;
}
// 8-bit kernel: int8 tiles and scales in q_*
static bool lstm_admits_q8(const bh_layer_t& d) {
    return d.quantize && d.in_size == d.out_size && bh_k_lstm_q8_units(d.out_size, bh::g_opt.lstm_q8_variant) != 0;
}

enum Handoff {
    HANDOFF_OUTPUT,   // peers poll the output tensor, which is filled with a sentinel first
    HANDOFF_RING,     // through a ring buffer of its own, armed by the launcher (ex16; q_ex for the 8-bit kernel)
    HANDOFF_LDS       // the ring lives in one workgroup
};
// Everything the engine needs to know to run one recurrent layer on a padded batch of Np chunks. Computed on demand: options may
// change between forwards (bh_encoder_set_option), and describe() must show what the next forward will do.
struct LstmPlan {
    bh_lstm_family family;          // the kernel of a launch (BH_LSTM_WGX2 only through pair_launch)
    const bh_lstm_instance* row = nullptr;      // the fp16 instance (null: BH_LSTM_Q8)
    const void* gate_w = nullptr;   // non-null: a GEMM writes the gate pre-activations first, with these weights / bias
    const float* gate_b = nullptr;
    Handoff handoff;
    bh_lstm_geometry geo;
    int n_rings, rings_per_launch;
    bool pairs;                     // wgx: more rings than one launch holds go two to a workgroup (wgx2) instead of into two launches
    bool pair_launch(int rings_left) const { return pairs && rings_per_launch > 0 && rings_left > rings_per_launch; }
};
static LstmPlan lstm_plan(const bh_encoder* e, const Layer& l, int Np) {
    const bh_layer_t& d = l.d;
    const int H = d.out_size;
    const bool regs = lstm_admits(d, BH_LSTM_WAVE);             // W_hh stays in registers (else: wide or streaming kernel)
    const bool q8 = l.q8 && (e->lstm_q8 || l.q8_only) && d.in_size == H;       // clears everything below
    const bool wide = !q8 && !regs && e->lstm_wide && lstm_admits(d, BH_LSTM_WIDE);
    const bool fused = !q8 && e->lstm_fused && lstm_admits(d, BH_LSTM_FUSED);
    const bool share = fused && e->lstm_fused >= 2 && lstm_admits(d, BH_LSTM_WGX);
    const bool cta = share && e->lstm_fused >= 3 && lstm_admits(d, BH_LSTM_CTA);
    const bool ring = e->lstm_exchange && e->ex16.p != nullptr;
    LstmPlan p;
    p.family = q8 ? BH_LSTM_Q8 : cta ? BH_LSTM_CTA : share && ring ? BH_LSTM_WGX : fused ? BH_LSTM_FUSED
               : wide ? BH_LSTM_WIDE : regs ? BH_LSTM_WAVE : BH_LSTM_STREAM;
    p.handoff = HANDOFF_RING;
    p.geo = bh_k_lstm_q8_geometry(H, l.q_variant);
    if (!q8) {
        p.row = lstm_admits(d, p.family, wide && !ring ? BH_LSTM_V_OUTPUT : 0);
        p.geo = p.row->geo;
        p.handoff = p.geo.unlimited ? HANDOFF_LDS : p.row->ex_bytes ? HANDOFF_RING : HANDOFF_OUTPUT;
        if (!p.row->projects) {
            p.gate_w = l.lstm_ih[p.row->w_ih].p;
            p.gate_b = (const float*)(p.row->w_ih == BH_LSTM_W_WIDE_ROWS ? l.lstm_bias_wide : l.b0).p;
        }
    }
    p.n_rings = Np / p.geo.ring_chunks;
    p.rings_per_launch = p.geo.rings_per_launch(e->n_cus);
    p.pairs = p.family == BH_LSTM_WGX && e->lstm_pair;
    return p;
}

// ---- bh_encoder_create, by layer kind ---------------------------------------------------------------------------------------------------
struct CreateState {
    int channels = 1, channels_eff = 1;     // features of the current activations, and as laid out in memory
    float bound = 4.0f;                     // their magnitude bound, for the static int8 input scale of a Q8-1 layer
    bool any_q8 = false;
};

static int create_conv(bh_encoder* e, size_t i, const bh_layer_t& d, CreateState& cs) {
    Layer& L = e->layers[i];
    BH_REQUIRE(d.w0 && d.in_size > 0 && d.out_size > 0 && d.winlen > 0 && d.stride > 0, "encoder_create: layer %zu: malformed convolution", i);
    BH_REQUIRE(d.groups <= 1, "encoder_create: layer %zu: grouped conv not supported here", i);
    const bool next_is_conv = next_kind(e, i) == BH_LAYER_CONV;      // does another convolution consume this output?
    const int K = d.winlen;
    L.cin_eff = d.in_size == 1 ? 1 : cs.channels_eff;
    L.cout_eff = next_is_conv ? pad8(d.out_size) : d.out_size;
    BH_REQUIRE(d.in_size == 1 || (cs.channels == d.in_size && L.cin_eff >= d.in_size),
               "encoder_create: layer %zu: convolution expects %d input channels, chain provides %d", i, d.in_size, cs.channels);
    std::vector<float> bpad((size_t)L.cout_eff, 0.0f);
    if (d.b0) for (int f = 0; f < d.out_size; ++f) bpad[f] = d.b0[f];
    L.pointwise = d.in_size != 1 && K == 1 && d.stride == 1 && d.padding == 0 && L.cin_eff == d.in_size &&
                  d.in_size % 8 == 0 && L.cout_eff == d.out_size && d.out_size % 8 == 0;
    BH_REQUIRE(!d.add_residual || L.pointwise, "encoder_create: layer %zu: only pointwise convolutions can add a residual", i);
    int rc;
    if (L.pointwise) {
        rc = upload_f16(L.w0, d.w0, (size_t)d.out_size * d.in_size);
    } else if (d.in_size == 1) {
        std::vector<float> wpad((size_t)L.cout_eff * K, 0.0f);
        for (int f = 0; f < d.out_size; ++f)
            for (int k = 0; k < K; ++k) wpad[(size_t)f * K + k] = d.w0[(size_t)f * K + k];
        rc = upload_f32(L.w0, wpad.data(), wpad.size());
    } else {
        std::vector<float> wpad((size_t)L.cout_eff * L.cin_eff * K, 0.0f);
        for (int f = 0; f < d.out_size; ++f)
            for (int c = 0; c < d.in_size; ++c)
                for (int k = 0; k < K; ++k)
                    wpad[((size_t)f * L.cin_eff + c) * K + k] = d.w0[((size_t)f * d.in_size + c) * K + k];
        std::vector<uint16_t> pk(bh_conv1d_packed_halves(L.cin_eff, L.cout_eff, K));
        rc = bh_conv1d_pack(wpad.data(), L.cin_eff, L.cout_eff, K, pk.data());
        if (!rc) rc = upload(L.w0, pk.data(), pk.size() * 2);
    }
    if (!rc) rc = upload_f32(L.b0, bpad.data(), bpad.size());
    cs.channels = d.out_size;
    cs.channels_eff = L.cout_eff;
    cs.bound = d.activation == BH_ACT_TANH ? 1.0f : 4.0f;       // oracle/lstm_q8_ref.py: SWISH_BOUND = 4
    return rc;
}

static int create_lstm(bh_encoder* e, size_t i, const bh_layer_t& d, CreateState& cs) {
    Layer& L = e->layers[i];
    const int H = d.out_size, I = d.in_size;
    BH_REQUIRE(d.w0 && d.w1 && H > 0 && I > 0, "encoder_create: layer %zu: malformed lstm", i);
    const std::vector<const bh_lstm_instance*> rows = lstm_admitted(d);
    // a width that only the 8-bit kernel has an instance for (144, 336) runs where the layer is quantised, and nowhere else
    BH_REQUIRE((!rows.empty() || lstm_admits_q8(d)) && I % 8 == 0,
               "encoder_create: layer %zu: lstm needs hidden %% 32 == 0 (<= 512) or %% 64 == 0 (<= 1024), or a quantised layer of a width "
               "the 8-bit kernel serves, insize %% 8 == 0 (got %d, %d)", i, H, I);
    L.q8_only = rows.empty();
    std::vector<float> b((size_t)4 * H);
    lstm_pack_bias(BH_LSTM_W_ROWS, d.b0, d.b1, H, b.data());
    int rc = upload_f32(L.b0, b.data(), b.size());
    // each layout once, however many of the admitted instances want it
    std::vector<uint16_t> pk((size_t)4 * H * std::max(H, I));
    for (const bh_lstm_instance* row : rows) {
        if (row->w_ih == BH_LSTM_W_TILES || row->w_hh == BH_LSTM_W_TILES) {
            BH_REQUIRE(L.lstm_mt == 0 || L.lstm_mt == row->mt, "encoder_create: layer %zu: two tile sizes for hidden size %d", i, H);
            L.lstm_mt = row->mt;
        }
        if (!rc && !L.lstm_ih[row->w_ih].p) {
            rc = lstm_pack(row->w_ih, row->mt, d.w0, H, I, pk.data());
            if (!rc) rc = upload(L.lstm_ih[row->w_ih], pk.data(), (size_t)4 * H * I * 2);
        }
        if (!rc && !L.lstm_hh[row->w_hh].p) {
            rc = lstm_pack(row->w_hh, row->mt, d.w1, H, H, pk.data());
            if (!rc) rc = upload(L.lstm_hh[row->w_hh], pk.data(), (size_t)4 * H * H * 2);
        }
        if (!rc && row->w_ih == BH_LSTM_W_WIDE_ROWS && !L.lstm_bias_wide.p) {
            lstm_pack_bias(row->w_ih, d.b0, d.b1, H, b.data());
            rc = upload_f32(L.lstm_bias_wide, b.data(), b.size());
        }
        e->batch_pad = std::max(e->batch_pad, row->geo.ring_chunks);        // (32: rings of the wide kernel)
    }
    if (!rc && lstm_admits_q8(d)) {       // Q8-1 tiles and scales
        const int U = bh_k_lstm_q8_units(H, bh::g_opt.lstm_q8_variant);
        const size_t tile_bytes = (size_t)4 * H * ((H + 63) / 64 * 64);
        std::vector<int8_t> pk(tile_bytes);
        std::vector<float> s_ih((size_t)4 * H), s_hh((size_t)4 * H);
        rc = bh_k_lstm_q8_pack(d.w0, H, U, pk.data(), s_ih.data());
        if (!rc) rc = upload(L.q_wih, pk.data(), pk.size());
        if (!rc) rc = bh_k_lstm_q8_pack(d.w1, H, U, pk.data(), s_hh.data());
        if (!rc) rc = upload(L.q_whh, pk.data(), pk.size());
        const float xs = (float)((double)cs.bound / 127.0);
        for (int j = 0; j < 4 * H; ++j) { s_ih[j] = s_ih[j] * xs; s_hh[j] = s_hh[j] / 127.0f; }
        if (!rc) rc = upload_f32(L.q_sx, s_ih.data(), s_ih.size());
        if (!rc) rc = upload_f32(L.q_sh, s_hh.data(), s_hh.size());
        L.q8 = true;
        L.q_variant = bh::g_opt.lstm_q8_variant;
        L.q_bound = cs.bound;
        cs.any_q8 = true;
    }
    cs.channels = cs.channels_eff = H;
    cs.bound = 1.0f;
    return rc;
}

// LINEAR_CRF, LINEAR and UPSAMPLE: an fp16 weight of `rows` x in_size and an optional bias
static int create_linear(Layer& L, const bh_layer_t& d, size_t rows) {
    int rc = upload_f16(L.w0, d.w0, rows * d.in_size);
    if (!rc && d.b0) rc = upload_f32(L.b0, d.b0, rows);
    return rc;
}

static int create_transformer(bh_encoder* e, size_t i, const bh_layer_t& d) {
    Layer& L = e->layers[i];
    const int D = d.in_size, F = d.dim_ff;
    BH_REQUIRE(d.w0 && d.w1 && d.w2 && d.w3 && d.w4 && d.w5 && D > 0 && F > 0 && d.nhead > 0 && D % d.nhead == 0 && D / d.nhead == 64 &&
                   D % 8 == 0 && F % 8 == 0,
               "encoder_create: layer %zu: transformer layer needs head_dim 64 and all weights", i);
    int rc = upload_f16(L.w0, d.w0, (size_t)3 * D * D);
    if (!rc && d.b0) rc = upload_f32(L.b0, d.b0, (size_t)3 * D);
    if (!rc) rc = upload_f16(L.w1, d.w1, (size_t)D * D);
    if (!rc && d.b1) rc = upload_f32(L.b1, d.b1, D);
    if (!rc) {   // fc1 rows interleaved (y_j, gate_j) for the SwiGLU epilogue of the GEMM
        std::vector<float> wi((size_t)2 * F * D);
        for (int j = 0; j < F; ++j) {
            memcpy(&wi[(size_t)(2 * j) * D], d.w2 + (size_t)j * D, sizeof(float) * D);
            memcpy(&wi[(size_t)(2 * j + 1) * D], d.w2 + (size_t)(F + j) * D, sizeof(float) * D);
        }
        rc = upload_f16(L.w2, wi.data(), wi.size());
    }
    if (!rc) rc = upload_f16(L.w3, d.w3, (size_t)D * F);
    if (!rc) rc = upload_f32(L.w4, d.w4, D);
    if (!rc) rc = upload_f32(L.w5, d.w5, D);
    return rc;
}

// RESIDUAL_PROJ (fp16 weight) and CTC_DECODER (fp32 weight): the bias is always present on the device, zero if the model has none
static int create_with_bias(Layer& L, const bh_layer_t& d, bool w_f16) {
    const size_t n = (size_t)d.out_size * d.in_size;
    int rc = w_f16 ? upload_f16(L.w0, d.w0, n) : upload_f32(L.w0, d.w0, n);
    if (rc) return rc;
    std::vector<float> b((size_t)d.out_size, 0.0f);
    if (d.b0) memcpy(b.data(), d.b0, sizeof(float) * d.out_size);
    return upload_f32(L.b0, b.data(), b.size());
}

// fold into the producing layer's epilogue
static int create_clamp(bh_encoder* e, size_t i, const bh_layer_t& d, CreateState& cs) {
    const int pk = i > 0 ? e->layers[i - 1].d.kind : 0;
    BH_REQUIRE(pk == BH_LAYER_CONV || pk == BH_LAYER_LINEAR_CRF || pk == BH_LAYER_LINEAR,
               "encoder_create: layer %zu: clamp must follow a convolution or linear layer", i);
    Layer& P = e->layers[i - 1];
    P.fused_clamp = true;
    P.clamp_lo = d.clamp_lo;
    P.clamp_hi = d.clamp_hi;
    cs.bound = std::max(fabsf(d.clamp_lo), fabsf(d.clamp_hi));
    return 0;
}

static int create_layer(bh_encoder* e, size_t i, const bh_layer_t& d, CreateState& cs) {
    Layer& L = e->layers[i];
    switch (d.kind) {
        case BH_LAYER_CONV: return create_conv(e, i, d, cs);
        case BH_LAYER_LSTM: return create_lstm(e, i, d, cs);
        case BH_LAYER_LINEAR_CRF:
            BH_REQUIRE(d.w0 && d.in_size > 0 && d.out_size > 0 && d.in_size % 8 == 0, "encoder_create: layer %zu: malformed linearcrfencoder", i);
            e->out_features = d.out_size;
            return create_linear(L, d, d.out_size);
        case BH_LAYER_LINEAR:
            BH_REQUIRE(d.w0 && d.in_size > 0 && d.out_size > 0 && d.in_size % 8 == 0 && d.out_size % 8 == 0 && cs.channels == d.in_size,
                       "encoder_create: layer %zu: linear needs in/out features %% 8 == 0 and %d input features (chain provides %d)", i,
                       d.in_size, cs.channels);
            cs.channels = cs.channels_eff = d.out_size;
            return create_linear(L, d, d.out_size);
        case BH_LAYER_TRANSFORMER: return create_transformer(e, i, d);
        case BH_LAYER_DWCONV:
            BH_REQUIRE(d.w0 && d.in_size > 0 && d.in_size % 8 == 0 && d.winlen > 0 && d.stride > 0 && cs.channels == d.in_size &&
                           cs.channels_eff == d.in_size,
                       "encoder_create: layer %zu: depthwise conv needs %d (multiple of 8) input channels, chain provides %d", i, d.in_size,
                       cs.channels);
            return upload_f32(L.w0, d.w0, (size_t)d.in_size * d.winlen);
        case BH_LAYER_RESIDUAL_PROJ:
            BH_REQUIRE(d.w0 && d.in_size % 8 == 0 && d.out_size % 8 == 0 && d.in_size > 0 && d.out_size > 0 && cs.channels == d.in_size &&
                           cs.channels_eff == d.in_size,
                       "encoder_create: layer %zu: residual projection shape mismatch", i);
            return create_with_bias(L, d, true);
        case BH_LAYER_CTC_DECODER:
            BH_REQUIRE(d.w0 && d.in_size % 8 == 0 && d.out_size >= 1 && d.out_size <= 8 && cs.channels == d.in_size,
                       "encoder_create: layer %zu: ctc decoder needs features %% 8 == 0 and <= 8 classes", i);
            e->out_features = d.out_size;
            return create_with_bias(L, d, false);
        case BH_LAYER_UPSAMPLE:
            BH_REQUIRE(d.w0 && d.in_size > 0 && d.scale_factor > 0 && d.in_size % 8 == 0, "encoder_create: layer %zu: malformed upsample", i);
            return create_linear(L, d, (size_t)d.scale_factor * d.in_size);
        case BH_LAYER_CLAMP: return create_clamp(e, i, d, cs);
        default: BH_REQUIRE(false, "encoder_create: layer %zu: kind %d is not supported by this build", i, d.kind);
    }
}

// Everything sized by the whole chain: activation rotation, exchange buffers, transformer workspace, timeout slots.
static int create_workspace(bh_encoder* e, const CreateState& cs) {
    const size_t n_layers = e->layers.size();
    const int last = e->layers[n_layers - 1].d.kind;
    BH_REQUIRE(last == BH_LAYER_LINEAR_CRF || last == BH_LAYER_CTC_DECODER ||
                   (n_layers >= 2 && last == BH_LAYER_CLAMP && e->layers[n_layers - 2].d.kind == BH_LAYER_LINEAR_CRF),
               "encoder_create: the chain must end in a linearcrfencoder (optionally followed by clamp) or a ctc decoder");
    const int Np = (e->max_batch + e->batch_pad - 1) / e->batch_pad * e->batch_pad;
    Walk w;
    if (walk(e, Np, e->max_chunk, &w)) return -2;
    const size_t ab = w.act_bytes;
    bool has_res = false;
    for (const auto& l : e->layers) has_res |= l.d.kind == BH_LAYER_RESIDUAL_PROJ;
    if (has_res && e->res.alloc(ab + 256)) return -1;
    // two consecutive recurrent layers that exchange through sentinel-filled output: rotate three buffers so the
    // next layer's sentinel fill can run beside the current layer's kernel
    for (size_t i = 0; i < n_layers; ++i)
        if (e->layers[i].d.kind == BH_LAYER_LSTM && next_kind(e, i) == BH_LAYER_LSTM) e->n_act = 3;
    if (e->n_act == 3) {
        // (the side stream itself is created on first use: a stream that exists but idles still takes a slot in the
        // round-robin mapping of streams onto hardware queues, which multi-lane runs of narrow models notice)
        if (e->act[2].alloc(ab + 256) || hipMemset(e->act[2].p, 0, e->act[2].bytes) != hipSuccess ||
            hipEventCreateWithFlags(&e->fill_ready, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e->fill_done, hipEventDisableTiming) != hipSuccess) {
            bh_set_error("encoder_create: sentinel pre-fill resources");
            return -1;
        }
    }
    if (cs.any_q8) {      // int8 activations (fragment order, hidden size padded to 64) and the exchange ring buffer
        if (e->q_act[0].alloc(ab + 256) || e->q_act[1].alloc(ab + 256) || e->q_ex.alloc((size_t)4 * (Np / 16) * 16 * 1024 + 256))
            return -1;
    }
    {   // exchange ring buffer of the fp16 recurrent kernels that hand off through one: [4 time slots][rings]
        size_t exb = 0;
        for (const auto& l : e->layers) {
            if (l.d.kind != BH_LAYER_LSTM) continue;
            for (const bh_lstm_instance* row : lstm_admitted(l.d)) exb = std::max(exb, (size_t)4 * (Np / row->geo.ring_chunks) * row->ex_bytes);
        }
        if (exb && e->ex16.alloc(exb + 256)) return -1;
    }
    if (e->act[0].alloc(ab + 256) || e->act[1].alloc(ab + 256) || e->gates.alloc(w.gate_bytes + 256) ||
        e->sig.alloc((size_t)Np * e->max_chunk * 2) || e->err.alloc(sizeof(int) * bh_encoder::ERR_SLOTS) ||
        e->lstm_ws.alloc(bh_k_lstm_ws_bytes(Np, 1024)))
        return -1;
    if (w.qkv_bytes) {   // transformer workspace
        if (e->t_qkv.alloc(w.qkv_bytes + 256) || e->t_mid.alloc(w.mid_bytes + 256) || e->t_a.alloc(w.model_bytes + 256) ||
            e->t_b.alloc(w.model_bytes + 256))
            return -1;
        // rotary table: angle = t * 10000^(-i/32), fp32 like flash_attn.layers.rotary
        std::vector<float> cs_table((size_t)w.max_tokens * 32 * 2);
        if (bh_rotary_table(w.max_tokens, 64, cs_table.data())) return -2;
        if (upload_f32(e->rot, cs_table.data(), cs_table.size())) return -1;
        e->rot_len = w.max_tokens;
    }
    if (hipHostMalloc((void**)&e->err_host, sizeof(int) * bh_encoder::ERR_SLOTS, hipHostMallocDefault) != hipSuccess) {
        bh_set_error("encoder_create: hipHostMalloc failed");
        return -1;
    }
    for (int i = 0; i < bh_encoder::ERR_SLOTS; ++i) e->err_host[i] = 0;
    e->cur_err = (int*)e->err.p;
    if (hipMemset(e->err.p, 0, sizeof(int) * bh_encoder::ERR_SLOTS) != hipSuccess || hipMemset(e->act[0].p, 0, e->act[0].bytes) != hipSuccess ||
        hipMemset(e->act[1].p, 0, e->act[1].bytes) != hipSuccess) {
        bh_set_error("encoder_create: hipMemset failed");
        return -1;
    }
    return 0;
}

}  // namespace

extern "C" int bh_encoder_create(const bh_layer_t* layers, int n_layers, int device, int max_batch,
                                 int max_chunk, bh_encoder_t** out) {
    BH_REQUIRE(layers && n_layers > 0 && out, "encoder_create: bad arguments");
    BH_REQUIRE(max_batch > 0 && max_chunk > 0, "encoder_create: max_batch/max_chunk must be positive");
    int ndev = 0;
    BH_CHECK_HIP(hipGetDeviceCount(&ndev));
    BH_REQUIRE(ndev > 0, "encoder_create: no HIP device visible -- the MI355X engine has no CPU fallback");
    BH_REQUIRE(device >= 0 && device < ndev, "encoder_create: device %d out of range (%d visible)", device, ndev);
    int prev = 0;
    BH_CHECK_HIP(hipGetDevice(&prev));
    BH_CHECK_HIP(hipSetDevice(device));
    auto* e = new bh_encoder();
    e->device = device;
    e->max_batch = max_batch;
    e->max_chunk = max_chunk;
    auto fail = [&](int code) {
        delete e;
        (void)hipSetDevice(prev);
        return code;
    };
    if (hipDeviceGetAttribute(&e->n_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        bh_set_error("encoder_create: cannot query CU count");
        return fail(-1);
    }
    e->layers.resize(n_layers);
    for (int i = 0; i < n_layers; ++i) e->layers[i].d = layers[i];       // (all of them first: a layer looks at the kind of its consumer)
    CreateState cs;
    for (int i = 0; i < n_layers; ++i) {
        if (int rc = create_layer(e, (size_t)i, layers[i], cs)) return fail(rc);
        bh_layer_t& d = e->layers[i].d;
        d.w0 = d.w1 = d.w2 = d.w3 = d.w4 = d.w5 = d.b0 = d.b1 = nullptr;
    }
    if (int rc = create_workspace(e, cs)) return fail(rc);
    (void)hipSetDevice(prev);
    *out = e;
    return 0;
}

extern "C" void bh_encoder_destroy(bh_encoder_t* enc) {
    if (!enc) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(enc->device);
    delete enc;
    (void)hipSetDevice(prev);
}

extern "C" int bh_encoder_output_shape(const bh_encoder_t* enc, int L, int* T, int* C, int* stride) {
    BH_REQUIRE(enc && L > 0, "encoder_output_shape: bad arguments");
    Walk w;
    if (walk(enc, 16, L, &w)) return -2;
    if (T) *T = w.T;
    if (C) *C = w.C;
    if (stride) {
        int s = 1;
        for (const auto& l : enc->layers) {
            if (l.d.kind == BH_LAYER_CONV || l.d.kind == BH_LAYER_DWCONV) s *= l.d.stride;
            else if (l.d.kind == BH_LAYER_UPSAMPLE && l.d.scale_factor > 0) s /= l.d.scale_factor;
        }
        *stride = s;
    }
    return 0;
}

namespace {
// Do the convolutions at layers i (raw signal in), j1, j2 form the front end conv_front3_kernel serves (conv.hip)? Clamp layers in
// between are folded into the convolutions (fused_clamp) and skipped.
static bool conv_front3_at(const bh_encoder* e, size_t i, size_t* j1, size_t* j2) {
    const size_t ib = next_layer(e, i), ic = next_layer(e, ib);
    if (next_kind(e, i) != BH_LAYER_CONV || next_kind(e, ib) != BH_LAYER_CONV) return false;
    const Layer &a = e->layers[i], &b = e->layers[ib], &c = e->layers[ic];
    if (a.d.in_size != 1 || a.pointwise || b.pointwise || c.pointwise || b.d.add_residual || c.d.add_residual) return false;
    // the layer behind conv3 must be the recurrent stack (time-major store), as for conv_ws_kernel's use today
    if (next_kind(e, ic) != BH_LAYER_LSTM) return false;
    if (!bh_k_conv_front3_ok(a.cout_eff, a.d.winlen, a.d.stride, b.cin_eff, b.cout_eff, b.d.winlen, b.d.stride, c.cin_eff, c.cout_eff,
                             c.d.winlen, c.d.stride))
        return false;
    if (a.d.out_size != b.d.in_size || b.d.out_size != c.d.in_size || c.cout_eff != c.d.out_size) return false;
    *j1 = ib;
    *j2 = ic;
    return true;
}
}  // namespace

// Human-readable list of the kernels the engine will launch per layer (one line each), e.g. for bench.py's roofline label.
extern "C" int bh_encoder_describe(const bh_encoder_t* e, char* buf, size_t n) {
    BH_REQUIRE(e && buf && n > 0, "encoder_describe: bad arguments");
    std::string out;
    char line[256];
    int li = 0;
    for (const auto& l : e->layers) {
        const bh_layer_t& d = l.d;
        switch (d.kind) {
            case BH_LAYER_CONV: {
                size_t fj1 = 0, fj2 = 0;
                const bool front = d.in_size == 1 && conv_front3_at(e, (size_t)li, &fj1, &fj2);
                snprintf(line, sizeof(line), "%d conv %d->%d k%d s%d: %s\n", li, d.in_size, d.out_size, d.winlen, d.stride,
                         l.pointwise ? "gemm (pointwise)" : front ? "conv_front3_kernel (this and the next two convolutions in one kernel)"
                         : d.in_size == 1 ? "conv_first_kernel" : "conv_igemm_kernel / conv_ws_kernel");
                break;
            }
            case BH_LAYER_LSTM: {
                // (at the batch the engine was created for: more rings than one launch holds are served two per workgroup)
                const LstmPlan p = lstm_plan(e, l, (e->max_batch + e->batch_pad - 1) / e->batch_pad * e->batch_pad);
                const int H = d.out_size;
                char k[128];
                if (p.family == BH_LSTM_Q8)
                    snprintf(k, sizeof(k), "lstm_layer_q8_kernel<%d,%d> (int8 W/x/h, i32 MFMA 16x16x64)", (H + 63) / 64, bh_k_lstm_q8_units(H, l.q_variant) / 4);
                else
                    snprintf(k, sizeof(k), "%s%s%s", p.row->projects ? "" : "gemm + ",
                             (p.pair_launch(p.n_rings) ? bh_k_lstm_find(BH_LSTM_WGX2, H, 0) : p.row)->name,
                             p.family == BH_LSTM_STREAM ? " (weight streaming)" : "");
                snprintf(line, sizeof(line), "%d lstm %d%s: %s\n", li, H, d.reverse ? " rev" : "", k);
                break;
            }
            case BH_LAYER_LINEAR_CRF: snprintf(line, sizeof(line), "%d linearcrfencoder %d->%d: gemm\n", li, d.in_size, d.out_size); break;
            case BH_LAYER_LINEAR: snprintf(line, sizeof(line), "%d linear %d->%d: gemm\n", li, d.in_size, d.out_size); break;
            case BH_LAYER_TRANSFORMER: {
                const bool ring = e->attn_ring && bh_k_attention_ring_serves(d.win_left, d.win_right);      // as forward_transformer dispatches
                snprintf(line, sizeof(line), "%d transformer d%d h%d ff%d: gemm (Wqkv%s, out_proj, fc1 SwiGLU, fc2) + %s + rmsnorm_residual_kernel\n",
                         li, d.in_size, d.nhead, d.dim_ff, ring ? " + rotary" : "", ring ? "attention_ring_kernel" : "attention_kernel");
                break;
            }
            case BH_LAYER_UPSAMPLE: snprintf(line, sizeof(line), "%d linearupsample x%d: gemm\n", li, d.scale_factor); break;
            case BH_LAYER_CLAMP: snprintf(line, sizeof(line), "%d clamp: fused into the previous layer's epilogue\n", li); break;
            case BH_LAYER_DWCONV: snprintf(line, sizeof(line), "%d dwconv k%d: dwconv_kernel\n", li, d.winlen); break;
            case BH_LAYER_RESIDUAL_PROJ: snprintf(line, sizeof(line), "%d residual projection: gemm\n", li); break;
            case BH_LAYER_CTC_DECODER: snprintf(line, sizeof(line), "%d ctc decoder: ctc_head_kernel\n", li); break;
            default: snprintf(line, sizeof(line), "%d kind %d\n", li, d.kind);
        }
        out += line;
        ++li;
    }
    snprintf(buf, n, "%s", out.c_str());
    return 0;
}

// ---- bh_encoder_forward, by layer kind --------------------------------------------------------------------------------------------------
namespace {

// Where a forward stands between two layers.
struct Cursor {
    const void* cur;                 // current activations, in layout `lay`: `len` positions of C features
    Layout lay = L_SIGNAL;
    int len, C = 1;
    int which = 0;                   // the activation buffer the next layer writes
    const void* cur_q = nullptr;     // output of a Q8-1 layer feeding the next one (int8, fragment order)
    int qi = 0;
    bool res_ready = false;          // a residual projection is pending in e->res
    int N, Np;                       // batch, and padded to whole rings
    hipStream_t st;
    void* scores;
    int n_act;
    void advance(void* dst) { cur = dst; which = (which + 1) % n_act; }
};

// Sentinel pre-fill for the recurrent layer that follows layer i (whose output buffer is act[which]): the buffer after
// it in the rotation is free once everything queued so far has run, so it is filled on the side stream while layer i's
// own kernels run. The next layer writes H_next features per (t, n) row into it.
static int prefill_next(bh_encoder* e, const Cursor& c, size_t i, size_t rows) {
    if (e->n_act != 3 || !e->lstm_prefill || e->profiling) return 0;
    const size_t j = next_layer(e, i);
    if (j >= e->layers.size() || e->layers[j].d.kind != BH_LAYER_LSTM) return 0;
    const Layer& nx = e->layers[j];
    if (lstm_plan(e, nx, c.Np).handoff != HANDOFF_OUTPUT) return 0;      // it exchanges elsewhere: nothing to pre-fill
    if (!e->fill_stream) BH_CHECK_HIP(hipStreamCreateWithFlags(&e->fill_stream, hipStreamNonBlocking));
    void* spare = e->act[(c.which + 1) % 3].p;
    BH_CHECK_HIP(hipEventRecord(e->fill_ready, c.st));
    BH_CHECK_HIP(hipStreamWaitEvent(e->fill_stream, e->fill_ready, 0));
    const int rc = bh_k_fill_u16(spare, 0xFFFFu, rows * nx.d.out_size, e->fill_stream);
    if (rc) return rc;
    BH_CHECK_HIP(hipEventRecord(e->fill_done, e->fill_stream));
    e->prefilled = spare;
    return 0;
}

// (i moves to the last convolution served when one kernel runs three of them)
static int forward_conv(bh_encoder* e, size_t& i, Cursor& c) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    hipStream_t st = c.st;
    const int Np = c.Np, len = c.len;
    BH_REQUIRE(c.lay == L_SIGNAL || c.lay == L_NLC, "encoder_forward: convolution after a time-major layer");
    BH_REQUIRE(c.C == d.in_size, "encoder_forward: layer %zu expects %d channels, got %d", i, d.in_size, c.C);
    size_t fj1 = 0, fj2 = 0;
    if (c.lay == L_SIGNAL && conv_front3_at(e, i, &fj1, &fj2)) {
        // conv1 -> conv2 -> conv3 in one kernel, the 16-channel intermediates stay in LDS (conv_front3_kernel)
        const Layer &l2 = e->layers[fj1], &l3 = e->layers[fj2];
        const int len1 = conv_out_len(len, d.winlen, d.stride, d.padding);
        const int len2 = conv_out_len(len1, l2.d.winlen, l2.d.stride, l2.d.padding);
        const int len3 = conv_out_len(len2, l3.d.winlen, l3.d.stride, l3.d.padding);
        BH_REQUIRE(len1 > 0 && len2 > 0 && len3 > 0, "encoder_forward: chunk too short for the convolution stack");
        void* dst3 = e->act[c.which].p;
        int rc3 = prefill_next(e, c, fj2, (size_t)len3 * Np);
        if (rc3) return rc3;
        ProfSpan span(e, st, BH_PROF_CONV);
        rc3 = bh_k_conv_front3(c.cur, Np, len, (const float*)l.w0.p, (const float*)l.b0.p, d.winlen, d.padding, d.activation, l.clamp_lo,
                               l.clamp_hi, l2.w0.p, (const float*)l2.b0.p, l2.d.winlen, l2.d.padding, l2.d.activation, l2.clamp_lo,
                               l2.clamp_hi, l3.w0.p, (const float*)l3.b0.p, l3.cout_eff, l3.d.winlen, l3.d.stride, l3.d.padding,
                               l3.d.activation, l3.clamp_lo, l3.clamp_hi, dst3, (long)l3.cout_eff, (long)Np * l3.cout_eff, st);
        if (rc3) return rc3;
        c.advance(dst3); c.len = len3; c.C = l3.d.out_size; c.lay = L_TNC;
        i = fj2;                        // (the two convolutions and the clamps between them are done)
        return 0;
    }
    const int lout = conv_out_len(len, d.winlen, d.stride, d.padding);
    void* dst = e->act[c.which].p;
    const bool tnc = next_kind(e, i) == BH_LAYER_LSTM;       // the consumer decides the output layout
    const int co = l.cout_eff;
    const long os_n = tnc ? co : (long)lout * co;
    const long os_t = tnc ? (long)Np * co : co;
    int rc;
    if (tnc) { rc = prefill_next(e, c, i, (size_t)lout * Np); if (rc) return rc; }
    ProfSpan span(e, st, BH_PROF_CONV);
    if (l.pointwise && !tnc) {
        const void* rsd = d.add_residual ? e->res.p : nullptr;
        BH_REQUIRE(!d.add_residual || c.res_ready, "encoder_forward: layer %zu adds a residual that was never projected", i);
        rc = bh_k_linear(c.cur, l.w0.p, (const float*)l.b0.p, dst, Np * len, d.out_size, d.in_size, d.in_size,
                         d.in_size, d.out_size, d.activation, 1.0f, l.clamp_lo, l.clamp_hi, 0, 0, 0, 0, 0, st, rsd, d.out_size);
        if (d.add_residual) c.res_ready = false;
    } else if (c.lay == L_SIGNAL)
        rc = bh_k_conv_first(c.cur, (const float*)l.w0.p, (const float*)l.b0.p, dst, Np, len, lout,
                             co, d.winlen, d.stride, d.padding, d.activation, l.clamp_lo, l.clamp_hi, os_n, os_t, st);
    else
        rc = bh_k_conv_igemm(c.cur, l.w0.p, (const float*)l.b0.p, dst, Np, len, lout, l.cin_eff,
                             co, d.winlen, d.stride, d.padding, d.activation, l.clamp_lo, l.clamp_hi, os_n, os_t, st);
    if (rc) return rc;
    c.advance(dst); c.len = lout; c.C = d.out_size; c.lay = tnc ? L_TNC : L_NLC;
    return 0;
}

static int forward_lstm_q8(bh_encoder* e, size_t i, Cursor& c, const LstmPlan& p) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    hipStream_t st = c.st;
    const int H = d.out_size, len = c.len, Np = c.Np, R = p.n_rings;
    const size_t tile = bh_k_lstm_q8_tile_bytes(H);
    void* dst = e->act[c.which].p;
    const size_t j = next_layer(e, i);
    const bool next_q8 = j < e->layers.size() && e->layers[j].d.kind == BH_LAYER_LSTM && lstm_plan(e, e->layers[j], Np).family == BH_LSTM_Q8;
    int rc;
    const void* xq = c.cur_q;
    if (!xq) {       // first quantised layer: fp16 rows -> int8 fragments with the static input scale
        ProfSpan span(e, st, BH_PROF_OTHER);
        rc = bh_k_quantise_rows(c.cur, e->q_act[c.qi].p, len, Np, H, R, l.q_bound, st);
        if (rc) return rc;
        xq = e->q_act[c.qi].p;
        c.qi ^= 1;
    }
    void* hq_out = next_q8 ? e->q_act[c.qi].p : nullptr;
    void* h16_out = next_q8 ? nullptr : dst;
    ProfSpan span(e, st, BH_PROF_LSTM_REC);
    rc = bh_k_lstm_q8_arm(e->q_ex.p, R, H, st);
    if (rc) return rc;
    for (int r0 = 0; r0 < R; r0 += p.rings_per_launch) {
        const int nr = std::min(p.rings_per_launch, R - r0);
        rc = bh_k_lstm_layer_q8((const char*)xq + (size_t)r0 * tile, l.q_wih.p, l.q_whh.p, (const float*)l.q_sx.p,
                                (const float*)l.q_sh.p, (const float*)l.b0.p,
                                hq_out ? (char*)hq_out + (size_t)r0 * tile : nullptr,
                                h16_out ? (char*)h16_out + (size_t)r0 * 16 * H * 2 : nullptr,
                                (char*)e->q_ex.p + (size_t)r0 * tile, len, Np, H, R, nr, d.reverse, e->cur_err, st,
                                (int*)e->lstm_ws.p, e->lstm_force_slow | e->lstm_tune << 8, l.q_variant, nullptr, (unsigned)bh::g_opt.lstm_max_spins);
        if (rc) return rc;
    }
    if (next_q8) { c.cur_q = hq_out; c.qi ^= 1; }
    else { c.cur_q = nullptr; c.advance(dst); }
    c.C = H;
    return 0;
}

static int forward_lstm(bh_encoder* e, size_t i, Cursor& c) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    hipStream_t st = c.st;
    BH_REQUIRE(c.lay == L_TNC, "encoder_forward: lstm needs time-major input");
    BH_REQUIRE(c.C == d.in_size, "encoder_forward: layer %zu expects %d features, got %d", i, d.in_size, c.C);
    const int H = d.out_size, len = c.len, Np = c.Np;
    const int M = len * Np;
    const LstmPlan p = lstm_plan(e, l, Np);
    BH_REQUIRE(p.rings_per_launch >= 1, "encoder_forward: device has too few CUs (%d) for hidden size %d", e->n_cus, H);
    if (p.family == BH_LSTM_Q8) return forward_lstm_q8(e, i, c, p);
    BH_REQUIRE(c.cur_q == nullptr, "encoder_forward: layer %zu would read int8 activations it cannot consume", i);
    int rc;
    void* dst = e->act[c.which].p;
    if (p.gate_w) {
        ProfSpan span(e, st, BH_PROF_LSTM_GEMM);
        rc = bh_k_linear(c.cur, p.gate_w, p.gate_b, e->gates.p, M, 4 * H, d.in_size, d.in_size, d.in_size, 4 * H, bh::ACT_NONE, 1.0f,
                         -INFINITY, INFINITY, 0, 0, 0, 0, 0, st);
        if (rc) return rc;
    }
    if (p.handoff == HANDOFF_OUTPUT) {      // exchange sentinel in the output tensor (the ring-in-a-workgroup kernel exchanges through
                                            // LDS only, the ring-buffer kernels through their own armed buffer)
        if (e->prefilled == dst) {          // filled beside the previous layer's kernel
            BH_CHECK_HIP(hipStreamWaitEvent(st, e->fill_done, 0));
        } else {
            ProfSpan span(e, st, BH_PROF_FILL);
            rc = bh_k_fill_u16(dst, 0xFFFFu, (size_t)M * H, st);
            if (rc) return rc;
        }
    }
    e->prefilled = nullptr;
    if (next_kind(e, i) == BH_LAYER_LSTM) { rc = prefill_next(e, c, i, (size_t)M); if (rc) return rc; }
    ProfSpan span(e, st, BH_PROF_LSTM_REC);
    bh_lstm_launch layer{};
    layer.family = p.family;
    layer.input = p.gate_w ? e->gates.p : c.cur;
    layer.w_ih = l.lstm_ih[p.row->w_ih].p; layer.w_hh = l.lstm_hh[p.row->w_hh].p; layer.bias = (const float*)l.b0.p;
    layer.h_out = dst;
    layer.ex = p.handoff == HANDOFF_RING ? e->ex16.p : nullptr;
    layer.T = len; layer.N = Np; layer.H = H;
    layer.R = layer.n_rings = p.n_rings;
    layer.reverse = d.reverse;
    layer.err_flag = e->cur_err; layer.xcc_ws = (int*)e->lstm_ws.p;
    layer.write_through = e->lstm_force_slow; layer.tune = e->lstm_tune;
    // (more rings than one launch holds: the ring-buffer kernel carries two rings per workgroup where the plan pairs)
    rc = bh_k_lstm_run_layer(layer, p.rings_per_launch, p.pairs, st);
    if (rc) return rc;
    c.advance(dst); c.C = H;
    return 0;
}

static int forward_linear_crf(bh_encoder* e, size_t i, Cursor& c) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    BH_REQUIRE(c.lay == L_TNC || c.lay == L_NLC, "encoder_forward: linearcrfencoder needs encoded input");
    BH_REQUIRE(c.C == d.in_size, "encoder_forward: layer %zu expects %d features, got %d", i, d.in_size, c.C);
    const float sc = d.scale != 0.0f ? d.scale : 1.0f;
    int rc;
    ProfSpan span(e, c.st, BH_PROF_CRF_LINEAR);
    if (c.lay == L_TNC)   // rows are (t, n): remap to the caller's [N][T][C], drop padding rows
        rc = bh_k_linear(c.cur, l.w0.p, (const float*)l.b0.p, c.scores, c.len * c.Np, d.out_size, d.in_size, d.in_size,
                         d.in_size, d.out_size, d.activation, sc, l.clamp_lo, l.clamp_hi, 0, c.Np, 1, c.len, c.N, c.st);
    else
        rc = bh_k_linear(c.cur, l.w0.p, (const float*)l.b0.p, c.scores, c.len * c.N, d.out_size, d.in_size, d.in_size,
                         d.in_size, d.out_size, d.activation, sc, l.clamp_lo, l.clamp_hi, 0, 0, 0, 0, 0, c.st);
    if (rc) return rc;
    c.C = d.out_size;
    return 0;
}

// feature-axis linear layer; rows keep their layout ((t, n) or (n, t))
static int forward_linear(bh_encoder* e, size_t i, Cursor& c) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    BH_REQUIRE(c.lay == L_TNC || c.lay == L_NLC, "encoder_forward: linear needs encoded input");
    BH_REQUIRE(c.C == d.in_size, "encoder_forward: layer %zu expects %d features, got %d", i, d.in_size, c.C);
    void* dst = e->act[c.which].p;
    ProfSpan span(e, c.st, BH_PROF_OTHER);
    int rc = bh_k_linear(c.cur, l.w0.p, (const float*)l.b0.p, dst, c.len * c.Np, d.out_size, d.in_size, d.in_size, d.in_size,
                         d.out_size, bh::ACT_NONE, 1.0f, l.clamp_lo, l.clamp_hi, 0, 0, 0, 0, 0, c.st);
    if (rc) return rc;
    c.advance(dst); c.C = d.out_size;
    return 0;
}

static int forward_transformer(bh_encoder* e, size_t i, Cursor& c) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    hipStream_t st = c.st;
    const int len = c.len, N = c.N;
    BH_REQUIRE(c.lay == L_NLC, "encoder_forward: transformer layer needs [N][T][D] input");
    BH_REQUIRE(c.C == d.in_size, "encoder_forward: layer %zu expects d_model %d, got %d", i, d.in_size, c.C);
    BH_REQUIRE(len <= e->rot_len, "encoder_forward: %d tokens exceed the rotary table (%d)", len, e->rot_len);
    const int D = d.in_size, F = d.dim_ff;
    const int M = N * len;            // batch-major: padded chunks sit behind the valid rows
    const float eps = d.eps > 0.0f ? d.eps : 1e-5f;
    int rc;
    // profile spans (measurement only): the attention kernel and fc1 each get a span of their own - ONE launch per span, so that a
    // roofline can name a kernel - the projections and norms around them share the two older classes
    // default: rotary + softmax scale in the Wqkv epilogue, persistent ring-buffer attention kernel; the
    // block-per-workgroup kernel (rotation applied while staging) serves wider windows and "attn_ring" = 0
    const bool ring = e->attn_ring && bh_k_attention_ring_serves(d.win_left, d.win_right);
    // DeepNorm residual alpha * x fused into the projection's epilogue (fp32 accumulator + alpha * x, one rounding); the norm
    // kernel then reads one tensor instead of two ("norm_fuse" 1; default 0 = the separate residual read in the norm kernel)
    const bool fuse = e->norm_fuse != 0;
    // y = norm(proj(x) + alpha * res): the residual goes into the projection's epilogue (fuse) or into the norm kernel
    auto proj_norm = [&](const void* x, const void* w, const float* b, int K, const void* res, const float* gain, void* y) {
        int r = bh_k_linear(x, w, b, e->t_b.p, M, D, K, K, K, D, bh::ACT_NONE, 1.0f, -INFINITY, INFINITY, 0, 0, 0, 0, 0, st,
                            fuse ? res : nullptr, fuse ? D : 0, fuse ? d.alpha : 1.0f);
        if (!r) r = bh_k_rmsnorm_residual(e->t_b.p, fuse ? nullptr : res, gain, y, M, D, d.alpha, eps, st);
        return r;
    };
    {
        ProfSpan span(e, st, BH_PROF_ATTENTION);
        if (ring)
            rc = bh_k_linear_qkv_rotary(c.cur, l.w0.p, (const float*)l.b0.p, e->t_qkv.p, M, D, D, (const float*)e->rot.p,
                                        len, 0.125f * 1.4426950408889634f, st);     // scores in log2 units
        else
            rc = bh_k_linear(c.cur, l.w0.p, (const float*)l.b0.p, e->t_qkv.p, M, 3 * D, D, D, D, 3 * D, bh::ACT_NONE,
                             1.0f, -INFINITY, INFINITY, 0, 0, 0, 0, 0, st);
        if (rc) return rc;
    }
    {
        ProfSpan span(e, st, BH_PROF_ATTENTION_CORE);
        if (ring)
            rc = bh_k_attention_prerotated(e->t_qkv.p, e->t_a.p, N, len, d.nhead, D / d.nhead, d.win_left, d.win_right, st);
        else
            rc = bh_k_attention(e->t_qkv.p, e->t_a.p, (const float*)e->rot.p, N, len, d.nhead, D / d.nhead,
                                d.win_left, d.win_right, st);
        if (rc) return rc;
    }
    {
        ProfSpan span(e, st, BH_PROF_ATTENTION);
        rc = proj_norm(e->t_a.p, l.w1.p, (const float*)l.b1.p, D, c.cur, (const float*)l.w4.p, e->t_a.p);
        if (rc) return rc;
    }
    void* dst = e->act[c.which].p;
    {
        ProfSpan span(e, st, BH_PROF_MLP_FC1);
        rc = bh_k_linear(e->t_a.p, l.w2.p, nullptr, e->t_mid.p, M, 2 * F, D, D, D, F, bh::ACT_NONE, 1.0f,
                         -INFINITY, INFINITY, 1, 0, 0, 0, 0, st);
        if (rc) return rc;
    }
    {
        ProfSpan span(e, st, BH_PROF_MLP);
        rc = proj_norm(e->t_mid.p, l.w3.p, nullptr, F, e->t_a.p, (const float*)l.w5.p, dst);
        if (rc) return rc;
    }
    c.advance(dst);
    return 0;
}

static int forward_dwconv(bh_encoder* e, size_t i, Cursor& c) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    BH_REQUIRE(c.lay == L_NLC && c.C == d.in_size, "encoder_forward: depthwise conv needs [N][L][%d] input", d.in_size);
    const int lout = conv_out_len(c.len, d.winlen, d.stride, d.padding);
    void* dst = e->act[c.which].p;
    ProfSpan span(e, c.st, BH_PROF_CONV);
    int rc = bh_k_dwconv(c.cur, (const float*)l.w0.p, dst, c.Np, c.len, lout, c.C, d.winlen, d.stride, d.padding, c.st);
    if (rc) return rc;
    c.advance(dst); c.len = lout;
    return 0;
}

static int forward_residual_proj(bh_encoder* e, size_t i, Cursor& c) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    BH_REQUIRE(c.lay == L_NLC && c.C == d.in_size, "encoder_forward: residual projection needs [N][L][%d] input", d.in_size);
    ProfSpan span(e, c.st, BH_PROF_CONV);
    int rc = bh_k_linear(c.cur, l.w0.p, (const float*)l.b0.p, e->res.p, c.Np * c.len, d.out_size, d.in_size, d.in_size,
                         d.in_size, d.out_size, bh::ACT_NONE, 1.0f, -INFINITY, INFINITY, 0, 0, 0, 0, 0, c.st);
    if (rc) return rc;
    c.res_ready = true;
    return 0;
}

static int forward_ctc_decoder(bh_encoder* e, size_t i, Cursor& c) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    BH_REQUIRE(c.lay == L_NLC && c.C == d.in_size, "encoder_forward: ctc decoder needs [N][T][%d] input", d.in_size);
    ProfSpan span(e, c.st, BH_PROF_CRF_LINEAR);
    int rc = bh_k_ctc_head(c.cur, (const float*)l.w0.p, (const float*)l.b0.p, c.scores, (long)c.N * c.len, d.in_size, d.out_size, c.st);
    if (rc) return rc;
    c.C = d.out_size;
    return 0;
}

static int forward_upsample(bh_encoder* e, size_t i, Cursor& c) {
    const Layer& l = e->layers[i];
    const bh_layer_t& d = l.d;
    BH_REQUIRE(c.lay == L_NLC && c.C == d.in_size, "encoder_forward: upsample needs [N][T][%d] input", d.in_size);
    const int D = d.in_size, sf = d.scale_factor;
    void* dst = e->act[c.which].p;
    ProfSpan span(e, c.st, BH_PROF_OTHER);
    int rc = bh_k_linear(c.cur, l.w0.p, (const float*)l.b0.p, dst, c.N * c.len, sf * D, D, D, D, sf * D, bh::ACT_NONE,
                         1.0f, -INFINITY, INFINITY, 0, 0, 0, 0, 0, c.st);
    if (rc) return rc;
    c.advance(dst); c.len *= sf;     // [N][T][s*D] viewed as [N][s*T][D]
    return 0;
}

}  // namespace

extern "C" int bh_encoder_forward(bh_encoder_t* e, const void* signal, int N, int L, void* scores, void* stream_) {
    BH_REQUIRE(e && signal && scores, "encoder_forward: null argument");
    BH_REQUIRE(N > 0 && N <= e->max_batch, "encoder_forward: batch %d outside 1..%d", N, e->max_batch);
    BH_REQUIRE(L > 0 && L <= e->max_chunk, "encoder_forward: chunk %d outside 1..%d", L, e->max_chunk);
    hipStream_t st = (hipStream_t)stream_;
    int prev = 0;
    BH_CHECK_HIP(hipGetDevice(&prev));
    if (prev != e->device) BH_CHECK_HIP(hipSetDevice(e->device));
    struct Restore {
        int prev, dev;
        ~Restore() { if (prev != dev) (void)hipSetDevice(prev); }
    } restore{prev, e->device};

    // this forward's timeout slot (see bh_encoder::ERR_SLOTS): harvest the flag of the forward that used it last, zero it on the stream
    {
        const long n = ++e->ticket;
        const int slot = (int)(n % bh_encoder::ERR_SLOTS);
        if (n - bh_encoder::ERR_SLOTS > e->checked.load()) e->sticky.fetch_or(((volatile int*)e->err_host)[slot]);
        ((volatile int*)e->err_host)[slot] = 0;
        e->cur_err = (int*)e->err.p + slot;
        BH_CHECK_HIP(hipMemsetAsync(e->cur_err, 0, sizeof(int), st));
    }
    const int Np = (N + e->batch_pad - 1) / e->batch_pad * e->batch_pad;
    // stage the batch into an engine-owned [Np][L] buffer whose padding rows are zero
    if (Np != N) BH_CHECK_HIP(hipMemsetAsync((char*)e->sig.p + (size_t)N * L * 2, 0, (size_t)(Np - N) * L * 2, st));
    BH_CHECK_HIP(hipMemcpyAsync(e->sig.p, signal, (size_t)N * L * 2, hipMemcpyDeviceToDevice, st));

    e->prefilled = nullptr;
    Cursor c;
    c.cur = e->sig.p; c.len = L; c.N = N; c.Np = Np; c.st = st; c.scores = scores; c.n_act = e->n_act;
    for (size_t i = 0; i < e->layers.size(); ++i) {
        int rc = 0;
        switch (e->layers[i].d.kind) {
            case BH_LAYER_CLAMP: continue;          // folded into its producer
            case BH_LAYER_CONV: rc = forward_conv(e, i, c); break;
            case BH_LAYER_LSTM: rc = forward_lstm(e, i, c); break;
            case BH_LAYER_LINEAR_CRF: rc = forward_linear_crf(e, i, c); break;
            case BH_LAYER_LINEAR: rc = forward_linear(e, i, c); break;
            case BH_LAYER_TRANSFORMER: rc = forward_transformer(e, i, c); break;
            case BH_LAYER_DWCONV: rc = forward_dwconv(e, i, c); break;
            case BH_LAYER_RESIDUAL_PROJ: rc = forward_residual_proj(e, i, c); break;
            case BH_LAYER_CTC_DECODER: rc = forward_ctc_decoder(e, i, c); break;
            case BH_LAYER_UPSAMPLE: rc = forward_upsample(e, i, c); break;
            default: BH_REQUIRE(false, "encoder_forward: unsupported layer kind %d", e->layers[i].d.kind);
        }
        if (rc) return rc;
    }
    // The persistent recurrent kernels raise this forward's slot on a spin timeout and then finish with invalid output. Mirror it
    // into pinned host memory behind this forward: whoever has observed the completion of this call on `st` (an event, a D2H copy
    // of decoded outputs, a synchronise) reads it without another round trip -- bh_encoder_error_flag_at(ticket).
    BH_CHECK_HIP(hipMemcpyAsync(e->err_host + (e->cur_err - (int*)e->err.p), e->cur_err, sizeof(int), hipMemcpyDeviceToHost, st));
    return 0;
}

extern "C" long bh_encoder_last_ticket(const bh_encoder_t* e) { return e ? e->ticket.load() : -1; }

extern "C" int bh_encoder_error_flag_at(const bh_encoder_t* e, long ticket) {
    if (!e || !e->err_host) return 0;
    const long cur = e->ticket.load();
    if (ticket < 0 || ticket > cur) return 0;
    if (cur - ticket >= bh_encoder::ERR_SLOTS) {
        bh_set_error("forward %ld is more than %d forwards old: its timeout flag has been recycled", ticket, bh_encoder::ERR_SLOTS);
        return -1;
    }
    const int flag = ((volatile const int*)e->err_host)[ticket % bh_encoder::ERR_SLOTS];
    if (flag) bh_set_error("device-side timeout in a persistent kernel (flag=%d, forward %ld): the scores of that forward are invalid", flag, ticket);
    return flag;
}

// The caller has dealt with the timeout of forward `ticket` (re-ran the batch): drop its flag, so that it is neither harvested into the
// engine-wide flag when the slot is recycled nor reported by bh_encoder_error_flag / bh_encoder_check (advisor finding, round 4: a
// successful retry left poll() poisoned for the life of the engine).
extern "C" int bh_encoder_ack(bh_encoder_t* e, long ticket) {
    BH_REQUIRE(e && e->err_host, "encoder_ack: null engine");
    const long cur = e->ticket.load();
    BH_REQUIRE(ticket >= 0 && ticket <= cur, "encoder_ack: forward %ld has not been issued (last %ld)", ticket, cur);
    if (cur - ticket >= bh_encoder::ERR_SLOTS) {
        bh_set_error("forward %ld is more than %d forwards old: its timeout flag has been recycled", ticket, bh_encoder::ERR_SLOTS);
        return -1;
    }
    ((volatile int*)e->err_host)[ticket % bh_encoder::ERR_SLOTS] = 0;
    return 0;
}

// flags of the forwards that bh_encoder_check has not reported yet (host side only: completed forwards whose copy has landed)
static int pending_flags(const bh_encoder_t* e) {
    int flag = e->sticky.load();
    const long cur = e->ticket.load();
    long lo = e->checked.load() + 1;
    if (lo < cur - bh_encoder::ERR_SLOTS + 1) lo = cur - bh_encoder::ERR_SLOTS + 1;
    if (lo < 0) lo = 0;
    for (long n = lo; n <= cur; ++n) flag |= ((volatile const int*)e->err_host)[n % bh_encoder::ERR_SLOTS];
    return flag;
}

extern "C" int bh_encoder_error_flag(const bh_encoder_t* e) {
    if (!e || !e->err_host) return 0;
    const int flag = pending_flags(e);
    if (flag) bh_set_error("device-side timeout in a persistent kernel (flag=%d): the scores of that forward are invalid", flag);
    return flag;
}

extern "C" int bh_encoder_check(bh_encoder_t* e, void* stream_) {
    BH_REQUIRE(e, "encoder_check: null engine");
    BH_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream_));
    const int flag = pending_flags(e);
    // reported: forget everything up to the most recent forward. (A forward still in flight on ANOTHER stream than `stream_` is
    // past this check; its flag stays readable through its ticket.)
    e->sticky.store(0);
    if (flag) bh_set_error("device-side timeout in a persistent kernel (flag=%d)", flag);
    e->checked.store(e->ticket.load());
    return flag;
}

extern "C" int bh_encoder_profile(bh_encoder_t* e, int enable) {
    BH_REQUIRE(e, "encoder_profile: null engine");
    e->profiling = enable != 0;
    return 0;
}
extern "C" int bh_encoder_profile_read(bh_encoder_t* e, float* ms, int* launches) {
    BH_REQUIRE(e && ms && launches, "encoder_profile_read: null argument");
    for (int i = 0; i < BH_PROF_CLASSES; ++i) { ms[i] = 0.0f; launches[i] = 0; }
    for (auto& s : e->spans) {
        BH_CHECK_HIP(hipEventSynchronize(s.b));
        float t = 0.0f;
        BH_CHECK_HIP(hipEventElapsedTime(&t, s.a, s.b));
        if (s.cls >= 0 && s.cls < BH_PROF_CLASSES) { ms[s.cls] += t; launches[s.cls] += 1; }
        (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b);
    }
    e->spans.clear();
    return 0;
}

// debug: copy the LSTM statistics block (tune bit 4) of the last launch to the host
extern "C" int bh_encoder_debug_read(bh_encoder_t* e, void* host, size_t bytes, size_t offset) {
    BH_REQUIRE(e && host && offset + bytes <= e->lstm_ws.bytes, "encoder_debug_read: out of range");
    BH_CHECK_HIP(hipMemcpy(host, (char*)e->lstm_ws.p + offset, bytes, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int bh_encoder_set_option(bh_encoder_t* e, const char* name, int value) {
    BH_REQUIRE(e && name, "encoder_set_option: null argument");
    if (!strcmp(name, "lstm_force_slow")) { e->lstm_force_slow = value & 1; return 0; }
    if (!strcmp(name, "lstm_fused")) { e->lstm_fused = value; return 0; }
    if (!strcmp(name, "attn_ring")) { e->attn_ring = value; return 0; }
    if (!strcmp(name, "lstm_wide")) { e->lstm_wide = value; return 0; }
    if (!strcmp(name, "lstm_prefill")) { e->lstm_prefill = value; return 0; }
    if (!strcmp(name, "lstm_q8")) { e->lstm_q8 = value; return 0; }
    if (!strcmp(name, "lstm_exchange")) { e->lstm_exchange = value; return 0; }
    if (!strcmp(name, "lstm_pair")) { e->lstm_pair = value; return 0; }
    if (!strcmp(name, "norm_fuse")) { e->norm_fuse = value; return 0; }
    if (!strcmp(name, "gemm_v1")) { bh::g_opt.gemm_path = value; return 0; }   // alias of the process-wide "gemm_path"
    if (!strcmp(name, "lstm_tune")) { e->lstm_tune = value; return 0; }
    BH_REQUIRE(false, "encoder_set_option: unknown option '%s'", name);
}
