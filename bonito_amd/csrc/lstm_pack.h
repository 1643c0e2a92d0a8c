// Host-side weight layouts of the recurrent kernels that take tiles (lstm.hip: wgx, wgx2, cta, wide), stated once for
// engine.cpp (create_lstm) and abi.cpp (bh_lstm_layer_family). The per-wave fragment order is bh_lstm_pack_whh (abi.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include "devbuf.h"

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

// Wide layer: tiles of 8 units (MT = 2), and W_ih / bias with permuted rows, so that the gate GEMM writes
// G[t][n][(slice*4 + q)*8 + gate*2 + m] for unit slice*8 + q*2 + m. w_ih is [4H][I]; wp receives [4H][I], bp [4H] = b0 + b1
// (either may be null).
constexpr int LSTM_WIDE_MT = 2;
static inline void lstm_wide_permute(const float* w_ih, const float* b0, const float* b1, int H, int I, float* wp, float* bp) {
    const int MT = LSTM_WIDE_MT;
    for (int s8 = 0; s8 < H / 8; ++s8)
        for (int q = 0; q < 4; ++q)
            for (int g = 0; g < 4; ++g)
                for (int m = 0; m < MT; ++m) {
                    const size_t dst = (((size_t)s8 * 4 + q) * 4 + g) * MT + m;
                    const size_t src = (size_t)g * H + s8 * 8 + q * MT + m;
                    memcpy(&wp[dst * I], w_ih + src * I, sizeof(float) * I);
                    bp[dst] = (b0 ? b0[src] : 0.0f) + (b1 ? b1[src] : 0.0f);
                }
}

}  // namespace
