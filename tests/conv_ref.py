"""Plain fp64 restatement of the convolution stage (bh_conv1d_first, bh_conv1d, bh_conv1d_front3 layer by layer, bh_dwconv1d) with a
per-element a-priori error bound: the reference of tests/test_gpu_conv.py, pinned by tests/test_conv_ref_cpu.py. Device-agnostic torch
(float64 on whatever device the inputs live on); no import of bonito_amd.

A call is described by a `Call`: kind "first" (Cin = 1, raw signal [N][Lin], fp32 weights [Cout][K]), "igemm" (channel-minor input
[N][Lin][Cin], weights [Cout][Cin][K] as the fp16 values the packer stores) or "dw" (depthwise, C = Cin = Cout, fp32 weights [C][K], no
bias / activation / clamp); N, Lin, Cin, Cout, K, stride, pad, act (0 none, 1 swish, 2 tanh, 3 ReLU), lo, hi, bias; layout "NTC" (row of
(n, t) = n * Lout + t) or "TNC" (row = t * N + n, what the recurrent stack reads); os_t >= Cout halves per output row.

The operation (include/bonito_hip.h):
    z[n][t][f]   = sum_{k, c} w[f][c][k] * in[n][t * stride + k - pad][c] + bias[f]        positions outside [0, Lin) count as zero
    out[row][f]  = fp16(clamp(act(z), lo, hi)),   Lout = (Lin + 2 pad - K) / stride + 1    (conv_out_len; Lin + 2 pad >= K here)

The bound, by the argument of tests/linear_ref.py. The kernels multiply exactly (fp16 x fp16 on the MFMA; fp32 x fp16 under fmaf), accumulate
in fp32 in SOME order, stay in fp32 through bias, activation and clamp and round ONCE to fp16. A sum of n + 1 terms (n products and the
bias; the final operations take the rest) in fp32 in any order is within (n + 4) u S of the exact value to first order, u = 2^-24,
S = the sum of the magnitudes of its terms, n = K * Cin ("igemm") or K ("first", "dw"):
    dz    = (n + 4) * 2^-24 * (sum_{k, c} |w| |in| + |bias|)
    d     = L * dz,  L = 1 (none, ReLU, tanh: 1-Lipschitz; so is the clamp), 1.1 (swish: sup |swish'| = 1.0998)
    bound = d + ulp_fp16(want),  ulp_fp16 floored at 2^-24
one whole fp16 ulp rather than the half ulp of a perfect rounding, because an fp32 error can move a value across a rounding boundary; the
other half ulp (2.4e-4 relative) also covers the exp-based sigmoid / tanh of csrc/common.h (~1e-7 relative). Nothing here is tuned.
"""
import torch

SENTINEL = 0x7E5A                # int16 view of an fp16 NaN payload: no result can equal it bit for bit
FRONT = 16                       # halves of guard in front of the first output row
SLACK_ROWS = 64                  # rows of guard behind the last output row
IN_GUARD = 256                   # halves of fp16 NaN in front of and behind the N * Lin * Cin input halves
INF = float("inf")
F64 = torch.float64
KINDS = ("first", "igemm", "dw")


def conv_out_len(L, K, stride, pad):
    assert L + 2 * pad - K >= 0 and stride > 0
    return (L + 2 * pad - K) // stride + 1


def lin_for(Lout, K, stride, pad, extra=0):
    """An input length that gives exactly `Lout` positions (+ `extra` < stride samples that change nothing)."""
    assert 0 <= extra < stride
    L = (Lout - 1) * stride + K - 2 * pad + extra
    assert L >= 1 and conv_out_len(L, K, stride, pad) == Lout
    return L


class Call:
    def __init__(self, kind, N, Lin, Cin, Cout, K, stride=1, pad=0, act=0, lo=-INF, hi=INF, bias=True, layout="NTC", os_t=None):
        assert kind in KINDS and layout in ("NTC", "TNC")
        self.kind, self.N, self.Lin, self.Cin, self.Cout, self.K, self.stride, self.pad = kind, N, Lin, Cin, Cout, K, stride, pad
        self.act, self.lo, self.hi, self.bias, self.layout = act, float(lo), float(hi), bool(bias) and kind != "dw", layout
        self.os_t = Cout if os_t is None else os_t
        self.Lout = conv_out_len(Lin, K, stride, pad)
        self.terms = K * Cin if kind == "igemm" else K
        assert self.os_t >= Cout
        assert kind != "first" or Cin == 1
        assert kind != "dw" or (Cin == Cout and act == 0 and not self.bias and self.lo == -INF and self.hi == INF
                                and layout == "NTC" and self.os_t == Cout)

    def __repr__(self):
        s = "%s(N=%d,Lin=%d,Cin=%d,Cout=%d,K=%d,s=%d,p=%d,act=%d" % (self.kind, self.N, self.Lin, self.Cin, self.Cout, self.K, self.stride,
                                                                    self.pad, self.act)
        if self.lo != -INF or self.hi != INF:
            s += ",clamp=%g:%g" % (self.lo, self.hi)
        return s + "%s,%s%s)" % ("" if self.bias or self.kind == "dw" else ",nobias", self.layout,
                                 ",os_t=%d" % self.os_t if self.os_t != self.Cout else "")

    # ---- output rows ----
    def abi_strides(self):
        """(os_n, os_t) as the C ABI takes them."""
        return (self.Lout * self.os_t, self.os_t) if self.layout == "NTC" else (self.os_t, self.N * self.os_t)

    def rows(self, device="cpu"):
        """int64 [N][Lout]: output row of (n, t)."""
        n = torch.arange(self.N, device=device)[:, None]
        t = torch.arange(self.Lout, device=device)[None, :]
        return n * self.Lout + t if self.layout == "NTC" else t * self.N + n

    def alloc_out(self, device):
        """The whole `out` allocation as int16 bits, pre-filled with the sentinel: FRONT halves, N * Lout rows, SLACK_ROWS rows."""
        return torch.full((FRONT + (self.N * self.Lout + SLACK_ROWS) * self.os_t,), SENTINEL, dtype=torch.int16, device=device)

    def out_view(self, buf):
        return buf[FRONT:].view(-1, self.os_t)

    def writable(self, device="cpu"):
        """bool [N * Lout + SLACK_ROWS][os_t]: the positions of `out` the call may write (the same set in both layouts)."""
        w = torch.zeros((self.N * self.Lout + SLACK_ROWS, self.os_t), dtype=torch.bool, device=device)
        w[:self.N * self.Lout, :self.Cout] = True
        return w

    # ---- input ----
    def alloc_in(self, x):
        """x [N][Lin][Cin] (any float type) -> flat fp16 buffer: IN_GUARD halves of NaN, the N * Lin * Cin values, IN_GUARD halves of NaN."""
        assert tuple(x.shape) == (self.N, self.Lin, self.Cin)
        buf = torch.full((2 * IN_GUARD + x.numel(),), float("nan"), dtype=torch.float16, device=x.device)
        buf[IN_GUARD:IN_GUARD + x.numel()] = x.reshape(-1).half()
        return buf

    def in_view(self, xbuf):
        return xbuf[IN_GUARD:IN_GUARD + self.N * self.Lin * self.Cin].view(self.N, self.Lin, self.Cin)


def ulp_fp16(v):
    """Spacing of fp16 at |v| (float64 tensor), floored at the subnormal spacing 2^-24."""
    _, e = torch.frexp(v.abs())                       # |v| = f * 2^e, f in [0.5, 1): the binade is 2^(e - 1), 10 fraction bits
    e = torch.where(v == 0, torch.full_like(e, -13), e)            # (frexp(0) has exponent 0)
    return torch.ldexp(torch.ones_like(v), (e - 11).clamp(min=-24))


def swish(z):
    return z * torch.sigmoid(z)


def act_fn(act, z):
    return {0: z, 1: swish(z), 2: torch.tanh(z), 3: torch.relu(z)}[act]


def _windows(c, xbuf, pos, dtype, zero_outside=True):
    """-> [N][Lout][K][Cin]: the input values at positions pos [Lout][K] of every batch item, read from the guarded flat buffer."""
    dev = xbuf.device
    n = torch.arange(c.N, device=dev)[:, None, None]
    flat = IN_GUARD + (n * c.Lin + pos[None]) * c.Cin
    idx = (flat[..., None] + torch.arange(c.Cin, device=dev)).clamp(0, xbuf.numel() - 1)
    g = xbuf[idx].to(dtype)
    if zero_outside:
        inside = (pos >= 0) & (pos < c.Lin)
        g = torch.where(inside[None, :, :, None], g, torch.zeros_like(g))
    return g


def _positions(c, device, pad=None, stride_on_tap=False):
    t = torch.arange(c.Lout, device=device)[:, None]
    k = torch.arange(c.K, device=device)[None, :]
    pad = c.pad if pad is None else pad
    return (t + k * c.stride - pad) if stride_on_tap else (t * c.stride + k - pad)


def weights3(c, w):
    """The weights of call `c` as [Cout][Cin][K] ("dw": [C][1][K])."""
    return w.reshape(c.Cout, 1, c.K) if c.kind in ("first", "dw") else w.reshape(c.Cout, c.Cin, c.K)


def reference(c, xbuf, w, bias=None):
    """-> (want, bound), float64 [N][Lout][Cout]. xbuf: the guarded input buffer of Call.alloc_in; w: fp32 ("first", "dw") or fp16-valued
    ("igemm") weights; bias fp32 [Cout] or None."""
    g = _windows(c, xbuf, _positions(c, xbuf.device), F64)                   # [N][Lout][K][Cin]
    w3 = weights3(c, w).to(F64)
    eq = "ntkc,ck->ntc" if c.kind == "dw" else "ntkc,fck->ntf"
    wk = w3[:, 0, :] if c.kind == "dw" else w3
    z = torch.einsum(eq, g, wk)
    S = torch.einsum(eq, g.abs(), wk.abs())
    if c.bias:
        z = z + bias.to(F64)
        S = S + bias.to(F64).abs()
    dz = (c.terms + 4) * 2.0 ** -24 * S
    want = act_fn(c.act, z).clamp(c.lo, c.hi)
    return want, (1.1 if c.act == 1 else 1.0) * dz + ulp_fp16(want)


def pack(c, w):
    """What bh_conv1d_pack writes for an "igemm" call: fp16 [Cout16][Kp], column k * Cin + c, zero elsewhere."""
    kp, c16 = -(-c.K * c.Cin // 32) * 32, -(-c.Cout // 16) * 16
    p = torch.zeros(c16, kp, dtype=torch.float16, device=w.device)
    p[:c.Cout, :c.K * c.Cin] = w.reshape(c.Cout, c.Cin, c.K).permute(0, 2, 1).reshape(c.Cout, -1).half()
    return p


DATA_CLASSES = ("normal", "big", "tiny")


def make_inputs(c, device, seed, cls="normal"):
    """-> dict(x [N][Lin][Cin] fp16, xbuf (guarded), w, bias). Seeded random values plus one asymmetric deterministic component, so that a
    permutation of positions, channels or taps shows. Classes (chosen so that the fp64 value itself stays a finite fp16, no Inf input):
      normal: |in| ~ 0.5, pre-activations ~ 1: every activation in its curved range, a clamp inside (-1, 1) bites
      big   : |in| ~ 4, pre-activations ~ 10 (max well below 65504): the model's clamp at 3.5 bites, swish ~ identity / zero, tanh saturated
      tiny  : |in| ~ 2^-9, outputs among the fp16 subnormals: the floor of the ulp term"""
    assert cls in DATA_CLASSES
    g = torch.Generator(device=device).manual_seed(seed)
    amp = {"normal": 0.5, "big": 4.0, "tiny": 2.0 ** -9}[cls]

    def ramp(shape, coef, mod, a):
        i = sum(torch.arange(s, device=device).reshape([-1 if j == d else 1 for j in range(len(shape))]) * coef[d] for d, s in enumerate(shape))
        return ((i % mod).float() - (mod - 1) / 2) * (a / mod)

    x = amp * (torch.randn(c.N, c.Lin, c.Cin, generator=g, device=device) + ramp((c.N, c.Lin, c.Cin), (131, 17, 5), 23, 0.7))
    wshape = (c.Cout, 1 if c.kind in ("first", "dw") else c.Cin, c.K)
    target = {"normal": 1.0, "big": 10.0, "tiny": 2.0 ** -13}[cls]          # spread of the pre-activation
    w = target / (amp * c.terms ** 0.5) *(torch.randn(wshape, generator=g, device=device) + ramp(wshape, (37, 11, 3), 19, 0.6))
    if c.kind == "igemm":
        w = w.half().float()                                # representable in fp16: the packer's rounding is pinned separately
    else:
        w = w.reshape(c.Cout, c.K)
    bias = None
    if c.bias:
        bias = {"normal": 0.5, "big": 3.0, "tiny": 2.0 ** -14}[cls] * torch.randn(c.Cout, generator=g, device=device)
    x = x.half()
    return {"x": x, "xbuf": c.alloc_in(x), "w": w.contiguous(), "bias": bias}


def verify(c, t, buf):
    """Compare the output allocation `buf` (int16 bits, from Call.alloc_out) of call `c` on inputs `t` with the reference: EVERY writable
    element against its bound, every other element against the sentinel. -> dict(bad, lost, clobbered, worst, at): `lost` writable
    elements still hold the sentinel (never written), `bad` were written but are outside the bound or not finite, `clobbered` elements
    outside the writable set lost their sentinel; `worst` = max err / bound over the written elements, at (n, t, f)."""
    dev = buf.device
    want, bound = reference(c, t["xbuf"], t["w"], t["bias"])
    out = c.out_view(buf)
    bits = out[c.rows(dev).reshape(-1), :c.Cout].reshape(c.N, c.Lout, c.Cout)
    got = bits.view(torch.float16).to(F64)
    unwritten = bits == SENTINEL
    ratio = (got - want).abs() / bound
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, INF))
    ratio = torch.where(unwritten, torch.zeros_like(ratio), ratio)
    k = int(ratio.argmax().item())
    at = (k // (c.Lout * c.Cout), k // c.Cout % c.Lout, k % c.Cout)
    rest = out.clone()
    rest[c.writable(dev)] = SENTINEL
    clobbered = int((rest != SENTINEL).sum().item()) + int((buf[:FRONT] != SENTINEL).sum().item())
    return {"bad": int((ratio > 1.0).sum().item()), "lost": int(unwritten.sum().item()), "clobbered": clobbered,
            "worst": float(ratio.max().item()), "at": at}


def ok(r):
    return r["bad"] == 0 and r["lost"] == 0 and r["clobbered"] == 0


def message(c, r, what=""):
    return ("%s %r: %d elements over the bound, worst err / bound %.3g at (n, t, f) = %r; %d writable elements never written; %d guard "
            "elements lost their sentinel" % (what, c, r["bad"], r["worst"], r["at"], r["lost"], r["clobbered"]))


# --------------------------------------------------------------------------------------------------------------------------------------
# float32 emulation of a correct kernel (and of subtly wrong ones): used by test_conv_ref_cpu.py only
DEFECTS = ("last_tap", "pad_off", "stride_tap", "pack_ck", "kpad_weight", "no_bias", "act_swap", "no_clamp", "last_block", "one_past",
           "layout_swap", "next_item")


def _fma(a, b, acc):
    """fmaf on float32 tensors: the product of two floats is exact in float64, the sum is rounded to float64 and then to float32 (a
    double rounding that differs from one rounding in ~2^-29 of the cases, by one fp32 ulp)."""
    return (a.double() * b.double() + acc.double()).float()


def emulate(c, t, buf, defect=None):
    """Write what a kernel would into `buf`, in each kernel's accumulation order: "first" an fmaf chain over the taps starting from the
    bias; "dw" an fmaf chain from zero; "igemm" k-steps of 32 columns (k * Cin + c, zero-padded to Kp) ascending into ONE fp32
    accumulator (the 32 exact products of a step summed in float64 and added with one rounding: the MFMA's inner order is not
    architected, and the bound does not depend on it), the bias added behind; activation and clamp in fp32, one rounding to fp16.
    `defect`: one of DEFECTS planted into it."""
    assert defect is None or defect in DEFECTS
    f32 = torch.float32
    pos = _positions(c, "cpu", pad=c.pad + 1 if defect == "pad_off" else None, stride_on_tap=defect == "stride_tap")
    g = _windows(c, t["xbuf"], pos, f32, zero_outside=defect != "next_item")        # [N][Lout][K][Cin]
    w3 = weights3(c, t["w"]).float().clone()
    if defect == "last_tap":
        w3[:, :, c.K - 1] = 0
    b = t["bias"].float() if (c.bias and defect != "no_bias") else torch.zeros(c.Cout)
    if c.kind in ("first", "dw"):
        acc = b.expand(c.N, c.Lout, c.Cout).contiguous() if c.kind == "first" else torch.zeros(c.N, c.Lout, c.Cout)
        for k in range(c.K):
            xk = g[:, :, k, :] if c.kind == "dw" else g[:, :, k, 0:1]
            acc = _fma(w3[:, 0, k].expand_as(acc), xk.expand_as(acc), acc)
        z = acc
    else:
        n, kp = c.K * c.Cin, -(-c.K * c.Cin // 32) * 32
        wp = torch.zeros(c.Cout, kp, dtype=f32)
        wp[:, :n] = w3.reshape(c.Cout, n) if defect == "pack_ck" else w3.permute(0, 2, 1).reshape(c.Cout, n)
        cols = torch.zeros(c.N, c.Lout, kp, dtype=f32)
        cols[:, :, :n] = g.reshape(c.N, c.Lout, n)
        if defect == "kpad_weight":
            assert kp > n
            wp[:, n] = 0.25
            tail = _windows(c, t["xbuf"], _positions(c, "cpu")[:, :1] + c.K, f32)           # the span continues with the next position
            cols[:, :, n] = tail[:, :, 0, 0]
        acc = torch.zeros(c.N, c.Lout, c.Cout, dtype=f32)
        for ks in range(kp // 32):
            step = torch.einsum("ntj,fj->ntf", cols[:, :, 32 * ks:32 * ks + 32].double(), wp[:, 32 * ks:32 * ks + 32].double())
            acc = (acc.double() + step).float()
        z = acc + b
    act = {1: 2, 2: 1, 0: 3, 3: 0}[c.act] if defect == "act_swap" else c.act
    y = {0: z, 1: z * torch.sigmoid(z), 2: torch.tanh(z), 3: torch.relu(z)}[act]
    if defect != "no_clamp":
        y = y.clamp(c.lo, c.hi)
    bits = y.half().view(torch.int16)
    out = c.out_view(buf)
    rows = c.rows()
    if defect == "layout_swap":
        n_, t_ = torch.arange(c.N)[:, None], torch.arange(c.Lout)[None, :]
        rows = t_ * c.N + n_ if c.layout == "NTC" else n_ * c.Lout + t_
    keep = torch.ones(c.N, c.Lout, dtype=torch.bool)
    if defect == "last_block":
        keep[:, (c.Lout - 1) // 64 * 64:] = False
    out[rows[keep], :c.Cout] = bits[keep]
    if defect == "one_past":                                   # position Lout of every batch item stored as well
        flat = buf[FRONT:]
        os_n, os_t = c.abi_strides()
        idx = (torch.arange(c.N)[:, None] * os_n + c.Lout * os_t + torch.arange(c.Cout)[None, :]).reshape(-1)
        flat[idx] = 0
    return buf
