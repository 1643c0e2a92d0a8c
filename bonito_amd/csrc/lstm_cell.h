// The LSTM cell of every fp16 recurrent kernel: the inference kernels of lstm.hip and the training forward of lstm_train.hip, which
// therefore publish the same h bits from the same pre-activations.
#pragma once
#include "common.h"

namespace bh {

// One cell update from the four gate pre-activations (torch order i, f, g, o). The contractions are spelled out so
// that every kernel variant produces the same bits for the same pre-activations; h is
// forced into [-1, 1] so that a non-finite value can never alias the exchange sentinel.
struct LstmCell {
    float ei, ef, eg, eo;      // exp(-i), exp(-f), exp(-2g), exp(-o) of the clamped pre-activations
    float h;
    __device__ __forceinline__ LstmCell(float ai, float af, float ag, float ao, float& c) {
        // Transcendental issue (quarter rate) is what the gate arithmetic costs, so the five activations share
        // reciprocals: with E_x = exp(-x),
        //     c' = c * sig(f) + sig(i) * tanh(g) = (c * Di * Dg + (1 - Eg2) * Df) / (Df * Di * Dg),   D_x = 1 + E_x, Eg2 = exp(-2g)
        //     h  = sig(o) * tanh(c')             = (1 - Ec2) / ((1 + Ec2) * Do)
        // i.e. 5 exp + 2 rcp instead of 5 + 5. Pre-activations are clamped to +-25 (sig(-25) = 1.4e-11, far below what h
        // can resolve) so that no product of three (1 + E) factors leaves the fp32 range.
        ei = __expf(-__builtin_amdgcn_fmed3f(ai, -25.0f, 25.0f));
        ef = __expf(-__builtin_amdgcn_fmed3f(af, -25.0f, 25.0f));
        eg = __expf(-2.0f * __builtin_amdgcn_fmed3f(ag, -12.5f, 12.5f));
        eo = __expf(-__builtin_amdgcn_fmed3f(ao, -25.0f, 25.0f));
        const float didg = __fmul_rn(1.0f + ei, 1.0f + eg);
        const float df = 1.0f + ef;
        const float num = __builtin_fmaf(c, didg, __fmul_rn(1.0f - eg, df));
        c = __fmul_rn(num, rcpf_(__fmul_rn(df, didg)));
        const float ec = __expf(-2.0f * __builtin_amdgcn_fmed3f(c, -12.5f, 12.5f));
        const float hv = __fmul_rn(1.0f - ec, rcpf_(__fmul_rn(1.0f + ec, 1.0f + eo)));
        h = (fabsf(hv) <= 1.0f) ? hv : 0.0f;
    }
    // the four activations one by one, from the same exponentials: what a training forward stores for its backward
    __device__ __forceinline__ float sig_i() const { return rcpf_(1.0f + ei); }
    __device__ __forceinline__ float sig_f() const { return rcpf_(1.0f + ef); }
    __device__ __forceinline__ float tanh_g() const { return __fmul_rn(1.0f - eg, rcpf_(1.0f + eg)); }
    __device__ __forceinline__ float sig_o() const { return rcpf_(1.0f + eo); }
};

// -> h; c is updated in place
__device__ __forceinline__ float lstm_cell(float ai, float af, float ag, float ao, float& c) { return LstmCell(ai, af, ag, ao, c).h; }

}  // namespace bh
