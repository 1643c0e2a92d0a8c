"""Plain fp64 restatement of one recurrent layer (bh_lstm_layer_family: the fp16 kernel families of csrc/lstm.hip) with a per-element
a-priori error bound: the reference of tests/test_gpu_lstm.py, pinned by tests/test_lstm_ref_cpu.py. Device-agnostic torch (float64 on
whatever device the inputs live on, so the long cases run their reference on the card); no import of bonito_amd.

Definition (torch.nn.LSTM, one layer, one direction; gate order i, f, g, o; h_0 = c_0 = 0; `reverse` runs the time loop backwards):
    a_t = x_t W_ih^T + h_{t-1} W_hh^T + b            (4H pre-activations, x / W / h fp16 values, b fp32)
    c_t = sig(f) c_{t-1} + sig(i) tanh(g)            h_t = sig(o) tanh(c_t),  published as fp16
`free_running` is that recurrence in fp64 from the inputs alone. `teacher_forced` computes step t from the h_{t-1} THE KERNEL ITSELF
published (the fp16 values it consumed) and carries c in fp64 from those steps, so errors do not compound chaotically and every
published h_t is judged on its own: it returns (want, bound), float64 [T][N][H].

The bound, u = 2^-24 (half an fp32 ulp, relative), e = 2^-23 (one fp32 ulp: the AMD ISA manual states 1 ulp for v_exp_f32 and v_rcp_f32,
the two instructions __expf and rcpf_ compile to; csrc/common.h relies on the same figure). First order throughout.

Pre-activation, per gate, S = sum of the magnitudes of the terms of the sum:
    fused, wgx, wgx2, cta: fp16 products are exact, fp32 accumulates 2H + 1 terms in some order:
        da = (2H + 2) u (sum|x w| + sum|h w| + |b|)
    wave, stream, wide (gemm=True): G = fp16(x W_ih^T + b) is part of the operation:
        da = (H + 4) u (sum|x w| + |b|)    the GEMM's dz as linear_ref states it, K = H
           + ulp_fp16(G)                   one whole ulp, as linear_ref takes for a stored fp16
           + (H + 2) u (sum|h w| + |G|)    H products and G in fp32 in some order

lstm_cell(), with E_x = exp(-x), D_x = 1 + E_x, E_g = exp(-2g), spelled as in lstm.hip:
    c' = fma(c, Di Dg, (1 - Eg) Df) * rcp(Df (Di Dg))        h = (1 - Ec) * rcp((1 + Ec) Do),  Ec = exp(-2 c')
  * __expf(y) = v_exp_f32(fl(y * fl(log2 e))): two roundings of an argument of size |y| log2 e move the result by 2 |y| u relative,
    the instruction adds e:  r(y) = 2 |y| u + e, with y = x (i, f, o; |x| <= 25) or 2 g, 2 c (|.| <= 12.5) after the clamp.
  * D_x = fl(1 + E_x): relative error dD_x = (E_x / D_x) r + u, and E_x / D_x = 1 - sig(x) (i, f, o), (1 - tanh g) / 2 (g, c).
  * Numerator: |c| Di Dg (dDi + dDg + u) + [Eg r(2g) + u |1 - Eg|] Df + |1 - Eg| Df (dDf + u) + u |num|; denominator, reciprocal and the
    last product: |c'| (dDf + dDi + dDg + 2u + e + u). Divided by Df Di Dg (sig and tanh are the exact ratios):
        e_c = |c| sig(f) (dDi + dDg + u) + sig(i) [(1 - tanh g)/2 r(2g) + u |tanh g|] + sig(i) |tanh g| (dDf + u)
              + |c'| (dDf + dDi + dDg + 4u + e)
              + (|c| + 1) sig(-25) + (1 - tanh 12.5)                    the clamps of the pre-activations (1.4e-11, 2.8e-11)
    and in the same way for the output
        e_h = sig(o) [(1 - tanh c)/2 r(2c) + u |tanh c|] + |h| [(1 - tanh c)/2 r(2c) + dDo + e + 3u] + sig(o) (1 - tanh 12.5) + sig(-25)
    (c itself is not clamped, only the argument of its tanh; the |h| <= 1 guard never fires on a correct result.)
Propagation: the actual forget gate contracts the carried error, which keeps the bound tight over hundreds of steps:
    E_c[t] = sig(f) E_c[t-1] + |c_{t-1}| sig'(f) da_f + |tanh g| sig'(i) da_i + sig(i) (1 - tanh^2 g) da_g + e_c
    bound  = sig(o) (1 - tanh^2 c) E_c + |tanh c| sig'(o) da_o + e_h + ulp_fp16(want)
one whole fp16 ulp rather than half, for the reason linear_ref gives: an fp32 error can move a value across a rounding boundary.
Nothing here is tuned.

Data classes (`make_case`), shared by the CPU and the GPU test. Weights uniform in +-1/sqrt(H), rounded to fp16:
    typical      x ~ N(0, 1) clipped at 4, bias N(0, 0.3)
    saturating   biases of +-30 on i, f, o and +-15 on g in eight sign patterns by unit (u % 8): every clamp is hit from both sides;
                 pattern 0 (all positive) lets c climb by one per step past the +-12.5 clamp inside tanh(c), pattern 1 mirrors it
    long_memory  forget bias +8, input-gate bias -4: c is carried for hundreds of steps
    zeros        x = 0, no bias: c = 0 and h = 0 exactly
    overflow     forget bias -70 with g -15 / +15 and i, o +30: (1 - Eg) Df and Df Dg pass the fp32 range unless f is clamped. (At +-30
                 no product of three factors does: e^30 e^30 e^25 = 1.1e36, so there the clamp cannot be told from its absence.)
"""
import math

import torch

F64 = torch.float64
U = 2.0 ** -24
E1 = 2.0 ** -23
SIG_M25 = 1.0 / (1.0 + math.exp(25.0))
TANH_GAP = 1.0 - math.tanh(12.5)
CLASSES = ("typical", "saturating", "long_memory", "zeros", "overflow")
SAT_SIGNS = ((1, 1, 1, 1), (1, 1, -1, 1), (-1, -1, -1, -1), (1, -1, 1, 1), (-1, 1, 1, 1), (1, 1, 1, -1), (0, 0, 0, 0), (1, -1, -1, 1))


def ulp_fp16(v):
    """Spacing of fp16 at |v| (float64 tensor), floored at the subnormal spacing 2^-24 (as linear_ref.ulp_fp16)."""
    _, e = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(e, -13), e)
    return torch.ldexp(torch.ones_like(v), (e - 11).clamp(min=-24))


def make_case(cls, T, N, H, seed=0, replicate=False):
    """-> x fp16 [T][N][H], w_ih, w_hh float32 [4H][H] (fp16 values), bias float32 [4H] or None. replicate: one chunk in every column."""
    g = torch.Generator().manual_seed(1000 * seed + CLASSES.index(cls))
    k = 1.0 / math.sqrt(H)
    w_ih = ((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).half().float()
    w_hh = ((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).half().float()
    x = torch.randn(T, 1 if replicate else N, H, generator=g).clamp(-4, 4).half()
    if replicate:
        x = x.expand(T, N, H).contiguous()
    bias = (torch.randn(4 * H, generator=g) * 0.3).float()
    b4 = bias.view(4, H)
    unit = torch.arange(H)
    if cls == "saturating":
        signs = torch.tensor(SAT_SIGNS, dtype=torch.float32)[unit % 8]              # [H][4]
        mag = torch.tensor([30.0, 30.0, 15.0, 30.0])
        sat = (signs * mag).T                                                        # [4][H]
        b4.copy_(torch.where(sat != 0, sat, b4))
    elif cls == "long_memory":
        b4[1] += 8.0
        b4[0] -= 4.0
    elif cls == "overflow":
        on = unit % 4 < 2
        b4[0][on], b4[1][on], b4[3][on] = 30.0, -70.0, 30.0
        b4[2][on] = torch.where(unit[on] % 2 == 0, torch.tensor(-15.0), torch.tensor(15.0))
    elif cls == "zeros":
        x = torch.zeros_like(x)
        bias = None
    return x, w_ih, w_hh, bias


def _flip(a, reverse):
    return a.flip(0) if reverse else a


def free_running(x, w_ih, w_hh, bias, reverse=False):
    """The recurrence in fp64 from the inputs alone -> h float64 [T][N][H]."""
    xs = _flip(x.to(F64), reverse)
    wi, wh = w_ih.to(F64), w_hh.to(F64)
    T, N, H = xs.shape
    gx = xs @ wi.T
    if bias is not None:
        gx = gx + bias.to(F64)
    h = torch.zeros(N, H, dtype=F64, device=x.device)
    c = torch.zeros_like(h)
    out = []
    for t in range(T):
        i, f, g, o = (gx[t] + h @ wh.T).split(H, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out.append(h)
    return _flip(torch.stack(out), reverse)


def teacher_forced(x, w_ih, w_hh, bias, h_pub, reverse=False, gemm=False):
    """-> (want, bound) float64 [T][N][H]: step t from the published h_pub of the step before (fp16 [T][N][H], the kernel's output)."""
    dev = x.device
    xs, hp = _flip(x.to(F64), reverse), _flip(h_pub.to(F64), reverse)
    wi, wh = w_ih.to(F64), w_hh.to(F64)
    T, N, H = xs.shape
    hprev = torch.cat((torch.zeros(1, N, H, dtype=F64, device=dev), hp[:-1]))
    ax, Sx = xs @ wi.T, xs.abs() @ wi.abs().T
    if bias is not None:
        ax, Sx = ax + bias.to(F64), Sx + bias.to(F64).abs()
    ah, Sh = hprev @ wh.T, hprev.abs() @ wh.abs().T
    a = ax + ah
    if gemm:
        da = (H + 4) * U * Sx + ulp_fp16(ax) + (H + 2) * U * (Sh + ax.abs())
    else:
        da = (2 * H + 2) * U * (Sx + Sh)
    c = torch.zeros(N, H, dtype=F64, device=dev)
    Ec = torch.zeros_like(c)
    want, bound = [], []
    for t in range(T):
        ai, af, ag, ao = a[t].split(H, dim=-1)
        di, df, dg, do = da[t].split(H, dim=-1)
        si, sf, so, tg = torch.sigmoid(ai), torch.sigmoid(af), torch.sigmoid(ao), torch.tanh(ag)
        r_i, r_f, r_o = (2 * v.abs().clamp(max=25.0) * U + E1 for v in (ai, af, ao))
        r_g = 4 * ag.abs().clamp(max=12.5) * U + E1
        dDi, dDf, dDo = (1 - si) * r_i + U, (1 - sf) * r_f + U, (1 - so) * r_o + U
        hg = (1 - tg) / 2
        dDg = hg * r_g + U
        cn = sf * c + si * tg
        e_c = (c.abs() * sf * (dDi + dDg + U) + si * (hg * r_g + U * tg.abs()) + si * tg.abs() * (dDf + U)
               + cn.abs() * (dDf + dDi + dDg + 4 * U + E1) + (c.abs() + 1) * SIG_M25 + TANH_GAP)
        Ec = sf * Ec + c.abs() * sf * (1 - sf) * df + tg.abs() * si * (1 - si) * di + si * (1 - tg * tg) * dg + e_c
        c = cn
        tc = torch.tanh(c)
        w = so * tc
        hc = (1 - tc) / 2
        r_c = 4 * c.abs().clamp(max=12.5) * U + E1
        e_h = so * (hc * r_c + U * tc.abs()) + w.abs() * (hc * r_c + dDo + E1 + 3 * U) + so * TANH_GAP + SIG_M25
        want.append(w)
        bound.append(so * (1 - tc * tc) * Ec + tc.abs() * so * (1 - so) * do + e_h + ulp_fp16(w))
    return _flip(torch.stack(want), reverse), _flip(torch.stack(bound), reverse)


def worst(got, want, bound):
    """-> (ratio, (t, n, unit)): the largest |got - want| / bound and where."""
    r = (got.to(F64) - want).abs() / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    k = int(r.argmax())
    T, N, H = r.shape
    return float(r.flatten()[k]), (k // (N * H), k // H % N, k % H)
