// The option table behind bh_set_option (abi.cpp): one row per process-wide knob - public name, member of bh::Options, default, how a
// value is normalised, one line of description. include/bonito_hip.h describes every row at length; tests/test_abi.py reads the names
// and defaults from the rows below (keep one row per line, name first) and holds the header's knob comment to them, both ways.
// Process-wide, not thread-safe (options.h).
#include "options.h"

#include <string.h>

namespace bh {

Options g_opt;

#define BH_OPT(name) #name, &Options::name
static constexpr OptionRow OPTION_TABLE[] = {
    {BH_OPT(gemm_path), 0, Norm::keep, "linear GEMM kernel families: 0 auto, 1 = v1 only, 2 = no 256-tile kernel, 3 = no four-wave kernel, 5 = four-wave wherever legal"},
    {BH_OPT(gemm_tile16), 1, Norm::flag, "four-wave GEMM K-tile stream: 1 = 16x16x32 MFMAs, 0 = 32x32x16 (agree to fp16 rounding)"},
    {BH_OPT(gemm_order), 1, Norm::flag, "four-wave GEMM work order in an XCD: 1 = feature groups fastest, 0 = token blocks fastest (same bytes)"},
    {BH_OPT(gemm_gf), 0, Norm::keep, "four-wave GEMM feature tiles per block: 0 automatic, else rounded down to 1 / 2 / 4 / 8 / 16 / 32 (same bytes)"},
    {BH_OPT(gemm_stagger), 0, Norm::keep, "start-phase stagger of the persistent GEMM kernels, 0 = off (same bytes; measured without effect)"},
    {BH_OPT(attn_waves), 0, Norm::keep, "ring attention waves per workgroup: 0 automatic, 8, 12 (same results)"},
    {BH_OPT(attn_version), 2, Norm::one_or_two, "ring attention kernel: 2 = current, 1 = the first ring kernel"},
    {BH_OPT(attn_expt), 0, Norm::keep, "timing experiments of the ring attention kernel (bit mask): RESULTS ARE WRONG ON PURPOSE unless 0"},
    {BH_OPT(beam_fork), -1, Norm::keep, "posterior scan next to the beam kernel on a helper stream: -1 auto, 0 never, 1 always"},
    {BH_OPT(beam_select), 0, Norm::keep, "beam top-W selection: 0 histogram + boundary ranking, 1 radix search (same beams)"},
    {BH_OPT(beam_fuse), -1, Norm::keep, "forward / posterior scan as a second wave of the beam kernel: -1 auto (<= 256 states), 0 never, 1 always"},
    {BH_OPT(beam_cpw), 0, Norm::keep, "chunks per workgroup of the fused beam kernel at 256 states: 0 automatic, 1, 2, 4 (same bytes)"},
    {BH_OPT(decode_nt), 0, Norm::keep, "non-temporal score loads in the decode scans: 0 off"},
    {BH_OPT(viterbi_quad), 1, Norm::keep, "CRF Viterbi: 1 = four states per thread where the layout allows, 0 = the one-state kernel everywhere"},
    {BH_OPT(conv_ws), 1, Norm::keep, "weight-stationary kernel for the 384- / 96-channel 19-tap convolution: 1 on, 0 = generic implicit GEMM"},
    {BH_OPT(conv_fs), 1, Norm::keep, "feature-split instances of the implicit-GEMM convolution: 1 on, 0 = position-split"},
    {BH_OPT(conv_fuse), 1, Norm::keep, "conv1 -> conv2 -> conv3 as one kernel: 1 = 384-channel stacks, 2 = also 96-channel, 0 = three kernels"},
    {BH_OPT(conv_lds_kb), 64, Norm::positive_or_def, "KiB of LDS a workgroup of the implicit-GEMM convolution may take for its input span"},
    {BH_OPT(conv_front_pipe), 1, Norm::keep, "fused front end of the 384-channel stacks: 1 = conv1 / conv2 of the next block beside conv3 (12-wave pipeline), 0 = phase after phase (same bytes)"},
    {BH_OPT(conv_front_wgs), 0, Norm::keep, "workgroups of the pipelined front end: 0 = one per CU, n > 0 caps the grid (same bytes; test hook, A/B)"},
    {BH_OPT(lstm_max_spins), 1000000, Norm::nonneg_or_def, "bound of the recurrent kernels' exchange spin loops (0: the first incomplete poll round is a timeout)"},
    {BH_OPT(lstm_q8_variant), 0, Norm::keep, "geometry of the 8-bit recurrent kernel, read at bh_encoder_create: 0, 1, 2"},
};
#undef BH_OPT

// the struct's defaults and the table's cannot disagree
static constexpr bool defaults_agree() {
    constexpr Options o{};
    for (const OptionRow& r : OPTION_TABLE)
        if (o.*r.member != r.def) return false;
    return true;
}
static_assert(defaults_agree(), "options.h and OPTION_TABLE state different defaults");
static_assert(sizeof(OPTION_TABLE) / sizeof(OPTION_TABLE[0]) == sizeof(Options) / sizeof(int), "every member of Options has exactly one row");

const OptionRow* find_option(const char* name) {
    for (const OptionRow& r : OPTION_TABLE)
        if (!strcmp(name, r.name)) return &r;
    return nullptr;
}

}  // namespace bh
