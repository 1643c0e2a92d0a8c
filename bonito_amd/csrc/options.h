// The process-wide knobs of bh_set_option (include/bonito_hip.h): one struct the launchers read, one table (options.cpp) that names,
// normalises and describes them. Process-wide and NOT thread-safe: plain ints, no atomics, no locks - set them while nothing else
// calls into the library. Measurement / tuning / test hooks; none has a reference counterpart.
#pragma once

namespace bh {

struct Options {
    // gemm.hip (gemm_plan)
    int gemm_path = 0;          // GemmPath: 0 auto, 1 / 2 / 3 forbid kernel families, 5 forces the four-wave kernel
    int gemm_tile16 = 1;        // gemm_w4_kernel's K-tile stream: 1 = 16x16x32 MFMAs, 0 = 32x32x16
    int gemm_order = 1;         // GemmArgs::w4_order
    int gemm_gf = 0;            // feature tiles per block of gemm_w4_kernel's work order as requested (0 = automatic; gemm_plan rounds)
    int gemm_stagger = 0;       // start-phase stagger of the persistent kernels, in units (gemm_plan converts)
    // attention.hip
    int attn_waves = 0;
    int attn_version = 2;
    int attn_expt = 0;
    // beam.hip, crf.hip
    int beam_fork = -1;
    int beam_select = 0;
    int beam_fuse = -1;
    int beam_cpw = 0;
    int decode_nt = 0;
    int viterbi_quad = 1;
    // conv.hip
    int conv_ws = 1;
    int conv_fs = 1;
    int conv_fuse = 1;
    int conv_lds_kb = 64;
    int conv_front_pipe = 1;    // conv_front3_pipe_kernel for the 384-channel stacks
    int conv_front_wgs = 0;     // cap of its grid (0 = one workgroup per CU)
    // lstm.hip, lstm_q8.hip, engine.cpp
    int lstm_max_spins = 1000000;     // never negative (the table's normalisation); the kernels take it as unsigned
    int lstm_q8_variant = 0;          // read by bh_encoder_create
};
extern Options g_opt;

// How bh_set_option turns the caller's value into the stored one.
enum class Norm {
    keep,               // v
    flag,               // v ? 1 : 0
    one_or_two,         // v == 1 ? 1 : 2
    positive_or_def,    // v > 0 ? v : the default
    nonneg_or_def       // v >= 0 ? v : the default
};
struct OptionRow {
    const char* name;       // the public name
    int Options::*member;
    int def;                // the default (checked against Options{} at compile time)
    Norm norm;
    const char* what;       // one line; says so where results are wrong on purpose
    int normalise(int v) const {
        switch (norm) {
            case Norm::flag: return v ? 1 : 0;
            case Norm::one_or_two: return v == 1 ? 1 : 2;
            case Norm::positive_or_def: return v > 0 ? v : def;
            case Norm::nonneg_or_def: return v >= 0 ? v : def;
            default: return v;
        }
    }
};
const OptionRow* find_option(const char* name);     // null: no such option

}  // namespace bh
