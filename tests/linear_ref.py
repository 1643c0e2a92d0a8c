"""Plain fp64 restatement of the linear-layer GEMM (bh_linear, bh_linear_residual, bh_linear_qkv_rotary) with a per-element a-priori
error bound: the reference of tests/test_gpu_linear.py, pinned by tests/test_linear_ref_cpu.py. Device-agnostic torch (float64 on whatever
device the inputs live on, so the large GPU cases never cross PCIe in fp64); no import of bonito_amd.

A call is described by a `Call`. Buffers are 2-D fp16 tensors with their leading dimensions: X [M][ldx], W [N][ldw], residual [M][ldres]
(only columns < K resp. < N are ever used), bias fp32 [N], rotary table fp32 [>= T][32][2] (cos, sin) as bh_rotary_table(T, 64) writes it.

Order of the operation (include/bonito_hip.h):
    z[m][n] = sum_k X[m][k] W[n][k] + bias[n] + res_scale * residual[m][n]            (residual indexed by the INPUT row m)
    rotary  : per head of 64 of the features [0, 2D), D = N / 3, position m % T, i = dim % 32:
              (x1, x2) -> (x1 cos_i - x2 sin_i, x1 sin_i + x2 cos_i); features [0, D) times qscale afterwards
    plain   : y = act(z) (0 none, 1 swish, 2 tanh, 3 ReLU)       gated: y[j] = z[2j] * swish(z[2j + 1])  (N / 2 columns)
    out[orow(m)][n] = fp16(clamp(y * scale, lo, hi)),  orow(m) = (m / row_div) * row_s_hi + (m % row_div) * row_s_lo, rows with
    m % row_div >= row_lim dropped (row_div = 0: identity, row_lim = 0: none dropped).

The bound. The kernels multiply fp16 values exactly, accumulate in fp32 in SOME order, stay in fp32 through the epilogue and round ONCE to
fp16. A sum of K + 3 terms (K products, bias, residual term; the residual product and the final operations take the rest) in fp32 in any
order is within (K + 4) u S of the exact value to first order, u = 2^-24, S = the sum of the magnitudes of its terms:
    dz    = (K + 4) * 2^-24 * (sum_k |x_mk| |w_nk| + |bias_n| + |res_scale * res_mn|)
    d     = L * dz * |scale|,  L = 1 (none, ReLU, tanh: 1-Lipschitz; so is the clamp), 1.1 (swish: sup |swish'| = 1.0998)
    gated : d = (|swish(g)| dz_y + 1.1 |y| dz_g) * |scale|                             (product rule)
    rotary: d = (dz_a + dz_b) * qscale for a rotated pair (|cos|, |sin| <= 1)
    bound = d + ulp_fp16(want),  ulp_fp16 floored at 2^-24
one whole fp16 ulp rather than the half ulp of a perfect rounding, because an fp32 error can move a value across a rounding boundary; the
other half ulp (2.4e-4 relative) also covers the exp-based sigmoid / tanh of csrc/common.h (~1e-7 relative). Nothing here is tuned.
"""
import math

import torch

SENTINEL = 0x7E5A                # int16 view of an fp16 NaN payload: no result can equal it bit for bit
FRONT = 16                       # halves of guard in front of the first output row
SLACK_ROWS = 64                  # rows of guard behind the last addressable output row
INF = float("inf")
F64 = torch.float64


class Call:
    def __init__(self, M, N, K, act=0, scale=1.0, lo=-INF, hi=INF, gated=0, bias=True, res_scale=None, row=(0, 0, 0, 0),
                 rot=None, ldx=None, ldw=None, ldo=None, ldres=None):
        self.M, self.N, self.K = M, N, K
        self.act, self.scale, self.lo, self.hi, self.gated, self.bias = act, float(scale), float(lo), float(hi), int(gated), bool(bias)
        self.res_scale = None if res_scale is None else float(res_scale)         # None: no residual
        self.row = tuple(row)
        self.rot = rot                                                           # None | (T, qscale): N = 3 D
        self.ncol = N // 2 if gated else N
        self.ldx = K if ldx is None else ldx
        self.ldw = K if ldw is None else ldw
        self.ldo = -(-self.ncol // 8) * 8 if ldo is None else ldo          # the ABI wants multiples of 8 halves
        self.ldres = -(-N // 8) * 8 if ldres is None else ldres
        assert self.ldx >= K and self.ldw >= K and self.ldo >= self.ncol and self.ldres >= N
        assert rot is None or (N % 192 == 0 and not gated and act == 0 and res_scale is None and self.row[0] == 0
                               and self.scale == 1.0 and self.lo == -INF and self.hi == INF)

    def __repr__(self):
        keys = ("M", "N", "K", "act", "scale", "lo", "hi", "gated", "bias", "res_scale", "row", "rot", "ldx", "ldw", "ldo", "ldres")
        return "Call(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in keys)

    # ---- rows ----
    def row_map(self, device="cpu"):
        """-> (orow [M] int64: output row of every input row, live [M] bool: the row is stored)."""
        m = torch.arange(self.M, device=device)
        div, s_hi, s_lo, lim = self.row
        if div <= 0:
            return m, torch.ones(self.M, dtype=torch.bool, device=device)
        lo = m % div
        live = lo < lim if lim > 0 else torch.ones_like(lo, dtype=torch.bool)
        return torch.div(m, div, rounding_mode="floor") * s_hi + lo * s_lo, live

    def rows_addressable(self):
        """1 + the largest output row ANY input row maps to, dropped rows included (a kernel that stored one stays inside the allocation)."""
        return int(self.row_map()[0].max().item()) + 1

    def alloc_out(self, device):
        """The whole `out` allocation as int16 bits, pre-filled with the sentinel: FRONT halves, the addressable rows, SLACK_ROWS rows."""
        n = FRONT + (self.rows_addressable() + SLACK_ROWS) * self.ldo
        return torch.full((n,), SENTINEL, dtype=torch.int16, device=device)

    def out_view(self, buf):
        return buf[FRONT:].view(-1, self.ldo)

    def writable(self, device="cpu"):
        """bool [rows_addressable + SLACK_ROWS][ldo]: the positions of `out` the call may write."""
        w = torch.zeros((self.rows_addressable() + SLACK_ROWS, self.ldo), dtype=torch.bool, device=device)
        orow, live = self.row_map(device)
        w[orow[live], :self.ncol] = True
        return w


def ulp_fp16(v):
    """Spacing of fp16 at |v| (float64 tensor), floored at the subnormal spacing 2^-24."""
    _, e = torch.frexp(v.abs())                       # |v| = f * 2^e, f in [0.5, 1): the binade is 2^(e - 1), 10 fraction bits
    e = torch.where(v == 0, torch.full_like(e, -13), e)            # (frexp(0) has exponent 0)
    return torch.ldexp(torch.ones_like(v), (e - 11).clamp(min=-24))


def swish(z):
    return z * torch.sigmoid(z)


def reference(c, X, W, bias=None, res=None, cs=None, rows=None):
    """-> (want, bound), float64 [len(rows)][ncol], for the input rows `rows` (int64 tensor; None = all) of call `c`."""
    dev = X.device
    ms = torch.arange(c.M, device=dev) if rows is None else rows
    x = X[ms, :c.K].to(F64)
    w = W[:, :c.K].to(F64)
    z = x @ w.T
    S = x.abs() @ w.abs().T
    if c.bias:
        z = z + bias.to(F64)
        S = S + bias.to(F64).abs()
    if c.res_scale is not None:
        r = float(torch.tensor(c.res_scale, dtype=torch.float32)) * res[ms, :c.N].to(F64)      # res_scale as the fp32 the ABI passes
        z = z + r
        S = S + r.abs()
    dz = (c.K + 4) * 2.0 ** -24 * S
    scale = float(torch.tensor(c.scale, dtype=torch.float32))
    if c.rot is not None:
        T, qscale = c.rot
        qscale = float(torch.tensor(qscale, dtype=torch.float32))
        D = c.N // 3
        tab = cs[ms % T].to(F64)                                                   # [m][32][2]
        cos, sin = tab[:, None, :, 0], tab[:, None, :, 1]                          # broadcast over heads
        zh = z[:, :2 * D].reshape(len(ms), 2 * D // 64, 2, 32)
        x1, x2 = zh[:, :, 0], zh[:, :, 1]
        rot = torch.stack((x1 * cos - x2 * sin, x1 * sin + x2 * cos), dim=2).reshape(len(ms), 2 * D)
        dh = dz[:, :2 * D].reshape(len(ms), 2 * D // 64, 2, 32)
        dpair = (dh[:, :, 0] + dh[:, :, 1])[:, :, None].expand(-1, -1, 2, -1).reshape(len(ms), 2 * D)
        qs = torch.ones(c.N, dtype=F64, device=dev)
        qs[:D] = qscale
        want = torch.cat((rot, z[:, 2 * D:]), dim=1) * qs
        d = torch.cat((dpair, dz[:, 2 * D:]), dim=1) * qs
    elif c.gated:
        y, g = z[:, 0::2], z[:, 1::2]
        want = y * swish(g) * scale
        d = (swish(g).abs() * dz[:, 0::2] + 1.1 * y.abs() * dz[:, 1::2]) * abs(scale)
    else:
        a = {0: z, 1: swish(z), 2: torch.tanh(z), 3: torch.relu(z)}[c.act]
        want = a * scale
        d = (1.1 if c.act == 1 else 1.0) * dz * abs(scale)
    want = want.clamp(c.lo, c.hi)
    return want, d + ulp_fp16(want)


def rotary_table(T, dim=64):
    """fp32 [T][dim / 2][2] = (cos, sin)(t * 10000^(-2 i / dim)): what bh_rotary_table(T, dim) computes (pinned in test_linear_ref_cpu.py)."""
    i = torch.arange(dim // 2, dtype=F64)
    ang = torch.arange(T, dtype=F64)[:, None] * torch.pow(torch.tensor(10000.0, dtype=F64), -2.0 * i / dim)[None, :]
    return torch.stack((torch.cos(ang), torch.sin(ang)), dim=-1).float()


def make_inputs(c, device, seed):
    """-> dict(X, W, bias, res, cs) for call `c`: seeded random values (x ~ 0.5, w ~ 0.2, bias ~ 1, residual ~ 1) plus one asymmetric
    deterministic component, so that a permutation of rows, features or K chunks shows; every padding column NaN."""
    g = torch.Generator(device=device).manual_seed(seed)

    def rnd(r, k):
        return torch.randn(r, k, generator=g, device=device)

    def ramp(r, k, a, b, mod, amp):
        i = torch.arange(r, device=device)[:, None] * a + torch.arange(k, device=device)[None, :] * b
        return ((i % mod).float() - (mod - 1) / 2) * (amp / mod)

    def padded(v, ld):
        buf = torch.full((v.shape[0], ld), float("nan"), dtype=torch.float16, device=device)
        buf[:, :v.shape[1]] = v.half()
        return buf

    t = {"bias": None, "res": None, "cs": None}
    t["X"] = padded(0.5 * rnd(c.M, c.K) + ramp(c.M, c.K, 131, 17, 23, 0.35), c.ldx)
    t["W"] = padded(0.2 * rnd(c.N, c.K) + ramp(c.N, c.K, 37, 5, 19, 0.15), c.ldw)
    if c.bias:
        t["bias"] = torch.randn(c.N, generator=g, device=device)
    if c.res_scale is not None:
        t["res"] = padded(rnd(c.M, c.N) + ramp(c.M, c.N, 3, 7, 13, 0.5), c.ldres)
    if c.rot is not None:
        t["cs"] = rotary_table(c.rot[0]).to(device)
    return t


def verify(c, t, buf, slab=8192):
    """Compare the output allocation `buf` (int16 bits, from Call.alloc_out) of call `c` on inputs `t` with the reference: EVERY writable
    element against its bound, every other element against the sentinel. -> dict(bad, worst, at, lost); `message(...)` formats it."""
    dev = buf.device
    out = c.out_view(buf)
    orow, live = c.row_map(dev)
    bad, worst, at = 0, 0.0, None
    for lo in range(0, c.M, slab):
        ms = torch.arange(lo, min(c.M, lo + slab), device=dev)
        ms = ms[live[ms]]
        if ms.numel() == 0:
            continue
        want, bound = reference(c, t["X"], t["W"], t["bias"], t["res"], t["cs"], rows=ms)
        got = out[orow[ms], :c.ncol].view(torch.float16).to(F64)
        ratio = (got - want).abs() / bound
        ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, INF))       # a NaN (the sentinel: never written) or inf is wrong
        bad += int((ratio > 1.0).sum().item())
        w = float(ratio.max().item())
        if w > worst or at is None:
            k = int(ratio.argmax().item())
            worst, at = max(w, worst), (int(ms[k // c.ncol].item()), k % c.ncol)
    rest = out.clone()
    rest[c.writable(dev)] = SENTINEL
    lost = int((rest != SENTINEL).sum().item()) + int((buf[:FRONT] != SENTINEL).sum().item())
    return {"bad": bad, "worst": worst, "at": at, "lost": lost}


def message(c, r, what=""):
    m, n = r["at"] if r["at"] is not None else (-1, -1)
    return ("%s %r: %d elements over the bound, worst err / bound %.3g at (m, n) = (%d, %d), m %% 256 = %d, n %% 256 = %d; %d guard elements "
            "lost their sentinel" % (what, c, r["bad"], r["worst"], m, n, m % 256, n % 256, r["lost"]))


# --------------------------------------------------------------------------------------------------------------------------------------
# float32 emulation of a correct kernel (and of subtly wrong ones): used by test_linear_ref_cpu.py only
DEFECTS = ("drop_chunk", "k_tail", "bias_next", "res_next", "res_outrow", "no_res_scale", "rot_sign", "rot_pos", "rot_qk", "swap_gate",
           "scale_first", "clamp_first", "store16", "store_dropped")


def emulate(c, t, buf, defect=None, seed=0):
    """Write what a kernel would into `buf`: fp32 accumulation of the K dimension in 8-half chunks in a shuffled order, the epilogue in fp32,
    one rounding to fp16. `defect`: one of DEFECTS planted into it."""
    assert defect is None or defect in DEFECTS
    f32 = torch.float32
    x, w = t["X"][:, :c.K].float(), t["W"][:, :c.K].float()
    M, N = c.M, c.N
    acc = torch.zeros(M, N, dtype=f32)
    order = torch.randperm(c.K // 8, generator=torch.Generator().manual_seed(seed)).tolist()
    lane_rows = (torch.arange(M) % 16 == 5)[:, None]
    for n_done, ch in enumerate(order):
        xc = x[:, 8 * ch:8 * ch + 8]
        if defect == "drop_chunk" and n_done == len(order) // 2:
            xc = torch.where(lane_rows, torch.zeros_like(xc), xc)          # one 8-half chunk of K skipped for one lane's rows
        acc.addmm_(xc, w[:, 8 * ch:8 * ch + 8].T)
    if defect == "k_tail":                                                 # the chunk behind K read instead of zero-filled: with ldx = K that
        xf, wf = t["X"].reshape(-1), t["W"].reshape(-1)                    # is the head of the next row (NaN padding where ldx > K)
        xi = (torch.arange(M)[:, None] * c.ldx + c.K + torch.arange(8)[None, :]) % xf.numel()
        wi = (torch.arange(N)[:, None] * c.ldw + c.K + torch.arange(8)[None, :]) % wf.numel()
        acc.addmm_(xf[xi].float(), wf[wi].float().T)
    z = acc
    if c.bias:
        b = t["bias"].float()
        z = z + (torch.roll(b, -1) if defect == "bias_next" else b)
    orow, live = c.row_map()
    if c.res_scale is not None:
        r = t["res"][:, :N].float()
        if defect == "res_next":
            r = torch.roll(r, -1, dims=1)
        if defect == "res_outrow":
            r = r[orow % M]
        z = z + (1.0 if defect == "no_res_scale" else torch.tensor(c.res_scale, dtype=f32)) * r
    scale = torch.tensor(c.scale, dtype=f32)
    if c.rot is not None:
        T, qscale = c.rot
        D = N // 3
        pos = torch.arange(M) if defect == "rot_pos" else torch.arange(M) % T
        tab = (rotary_table(M) if defect == "rot_pos" else t["cs"])[pos]
        cos, sin = tab[:, None, :, 0], tab[:, None, :, 1]
        zh = z[:, :2 * D].reshape(M, 2 * D // 64, 2, 32)
        x1, x2 = zh[:, :, 0], zh[:, :, 1]
        sgn = -1.0 if defect == "rot_sign" else 1.0
        rot = torch.stack((x1 * cos - x2 * sin, sgn * x1 * sin + x2 * cos), dim=2).reshape(M, 2 * D)
        qs = torch.ones(N, dtype=f32)
        qs[:2 * D if defect == "rot_qk" else D] = qscale
        y = torch.cat((rot, z[:, 2 * D:]), dim=1) * qs
    elif c.gated:
        a, g = (z[:, 1::2], z[:, 0::2]) if defect == "swap_gate" else (z[:, 0::2], z[:, 1::2])
        y = (a * (g * torch.sigmoid(g)) * scale).clamp(c.lo, c.hi)
    else:
        def act(v):
            return {0: v, 1: v * torch.sigmoid(v), 2: torch.tanh(v), 3: torch.relu(v)}[c.act]
        if defect == "scale_first":
            y = act(z * scale).clamp(c.lo, c.hi)
        elif defect == "clamp_first":
            y = act(z).clamp(c.lo, c.hi) * scale
        else:
            y = (act(z) * scale).clamp(c.lo, c.hi)
    bits = y.half().view(torch.int16)
    out = c.out_view(buf)
    keep = torch.ones_like(live) if defect == "store_dropped" else live
    out[orow[keep], :c.ncol] = bits[keep]
    if defect == "store16":                                                # a 16-feature vector stored where only N % 16 features exist
        flat = buf[FRONT:]
        n16 = -(-c.ncol // 16) * 16
        idx = orow[live][:, None] * c.ldo + torch.arange(c.ncol, n16)[None, :]
        flat[idx.reshape(-1)] = 0
    return buf
