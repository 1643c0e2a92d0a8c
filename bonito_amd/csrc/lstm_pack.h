// Host-side weight layouts of the recurrent kernels (kernels.h: bh_lstm_layout), stated once for engine.cpp (create_lstm) and
// abi.cpp (bh_lstm_layer_family): lstm_pack / lstm_pack_bias. The per-wave fragment order is bh_lstm_pack_whh (abi.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include "devbuf.h"
#include "kernels.h"

namespace {      // (internal to each translation unit that includes this)

// Tile packing for the workgroup-shared LSTM kernel: [slice][tile m][kstep][lane][8] with U = 4*MT units per slice;
// row r of tile m is (unit slice*U + (r>>2)*MT + m, gate r&3), so the MFMA result leaves all four gate
// pre-activations of MT consecutive units in one lane. w is [4H][H] in torch gate order (W_hh, or W_ih when
// insize == H).
static inline int lstm_pack_tiles(const float* w, int H, int MT, uint16_t* packed) {
    const int U = 4 * MT, nks = H / 32, nsl = H / U;
    for (int s = 0; s < nsl; ++s)
        for (int m = 0; m < MT; ++m)
            for (int ks = 0; ks < nks; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int r = lane & 15;
                        const int row = (r & 3) * H + s * U + (r >> 2) * MT + m;
                        const int col = ks * 32 + (lane >> 4) * 8 + j;
                        packed[((((size_t)s * MT + m) * nks + ks) * 64 + lane) * 8 + j] = f2h(w[(size_t)row * H + col]);
                    }
    return 0;
}

// Wide layer: its gate GEMM writes G[t][n][(slice*4 + q)*8 + gate*2 + m] for unit slice*8 + q*2 + m (slices of 8 units, tiles of
// BH_LSTM_WIDE_MT = 2). The torch row (gate*H + unit) that row `dst` of the permuted W_ih / bias holds:
static inline size_t lstm_wide_row(int H, size_t dst) {
    const int MT = BH_LSTM_WIDE_MT;
    const size_t m = dst % MT, g = dst / MT % 4, q = dst / (4 * MT) % 4, s8 = dst / (16 * MT);
    return g * H + s8 * 8 + q * MT + m;
}

// fp32 weights w [4H][I] in torch gate order -> fp16 in layout L, 4 * H * I halves. FRAGS and TILES (of 4 * MT units) take I == H.
static inline int lstm_pack(bh_lstm_layout L, int MT, const float* w, int H, int I, uint16_t* packed) {
    switch (L) {
        case BH_LSTM_W_FRAGS: return I == H ? bh_lstm_pack_whh(w, H, packed) : -2;
        case BH_LSTM_W_TILES: return I == H && MT > 0 ? lstm_pack_tiles(w, H, MT, packed) : -2;
        default:
            for (size_t r = 0; r < (size_t)4 * H; ++r) {
                const float* src = w + (L == BH_LSTM_W_WIDE_ROWS ? lstm_wide_row(H, r) : r) * I;
                for (int c = 0; c < I; ++c) packed[r * I + c] = f2h(src[c]);
            }
            return 0;
    }
}
// b0 + b1 [4H] (either may be null) in the row order of W_ih layout L
static inline void lstm_pack_bias(bh_lstm_layout L, const float* b0, const float* b1, int H, float* bias) {
    for (size_t r = 0; r < (size_t)4 * H; ++r) {
        const size_t src = L == BH_LSTM_W_WIDE_ROWS ? lstm_wide_row(H, r) : r;
        bias[r] = (b0 ? b0[src] : 0.0f) + (b1 ? b1[src] : 0.0f);
    }
}

}  // namespace
