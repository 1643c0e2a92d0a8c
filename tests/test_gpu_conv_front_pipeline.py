"""The pipelined fused front end (`conv_front3_pipe_kernel`, "conv_front_pipe" 1: four producer waves compute conv1 / conv2 of the next
256-position block into a second LDS span buffer while eight consumer waves run conv3 of the current one; a workgroup walks a contiguous
run of (chunk, block) pairs) writes conv3's WHOLE allocation - guards, padding columns and sentinel included - bit for bit as

  (a) the phase-after-phase fused kernel ("conv_front_pipe" 0), and
  (b) the three separate kernels (what "conv_fuse" 0 runs), which tests/test_gpu_conv.py verifies element by element against fp64.

Shapes are the smallest at which the pipeline can go wrong: L3 of one block, a last block of one position, two and three blocks per
chunk plus one position (both buffer parities), N of 1 and 3 (a run crosses a chunk boundary), and grids capped by "conv_front_wgs" at
1, 2 and 3 workgroups (runs of every length from one block up, uneven splits) next to the automatic grid (one block per workgroup at
these sizes). The other factors (K1, K2, stride, pads, epilogue kinds of test_gpu_conv._front3_cases) cycle with the case index."""
import functools

import pytest
import torch

import conv_ref as cr
import test_gpu_conv as tc
from bonito_amd import _lib

pytestmark = pytest.mark.gpu
PIPE_DEFAULTS = dict(conv_front_pipe=1, conv_front_wgs=0)
E = [dict(act=1, **tc.S35), dict(act=2), dict(act=3, bias=False), dict(act=0, **tc.IN1), dict(act=1)]      # as test_gpu_conv._front3_cases
L3S, NS, WGS = (1, 17, 256, 257, 513, 769), (1, 3), (1, 2, 3, 0)


def _shapes():
    out, i = [], 0
    for L3 in L3S:
        for N in NS:
            i += 1
            K1, K2, K3, s3 = (5, 3)[i % 2], (5, 1, 6)[i % 3], (19, 20)[i // 2 % 2], (6, 5, 7)[i // 2 % 3]
            p1, p2, p3 = (K1 // 2, 0)[i // 2 % 2], (K2 // 2, 0)[i // 3 % 2], (K3 // 2, 0)[i // 4 % 2]
            while (L3 - 1) * s3 + K3 - 2 * p3 + K2 - 1 - 2 * p2 < 1:       # the largest conv3 pad under which conv1 has an output
                p3 -= 1
            out.append((N, L3, K1, K2, K3, s3, p1, p2, p3, E[i % 5], E[(i + 1) % 5], E[(i + 2) % 5]))
    # the hac model's own layers on three blocks and on one partial block
    out.append((3, 513, 5, 5, 19, 6, 2, 2, 9, E[0], E[0], E[0]))
    out.append((1, 17, 5, 5, 19, 6, 2, 2, 9, E[0], E[0], E[0]))
    return out


def _sid(v):
    return "N%d-L3_%d-K%d_%d_%d-s%d-p%d_%d_%d-a%d%d%d" % (v[:9] + (v[9]["act"], v[10]["act"], v[11]["act"]))


def _fused(layers, t, opts):
    """conv3's allocation after bh_conv1d_front3 under `opts` (restored behind the call)."""
    c1, c2, c3 = layers
    buf = c3.alloc_out(tc.dev())
    try:
        tc._set(opts)
        rc = tc._front3_call(c1, c2, c3, t[0], t[1], t[2], buf.data_ptr() + 2 * cr.FRONT)
        _lib.check(rc, "bh_conv1d_front3 %r" % (opts,))
        assert _lib.lib().bh_conv1d_last_kernel() == tc.K_F384
    finally:
        tc._set(PIPE_DEFAULTS)
    return buf


@functools.lru_cache(maxsize=None)
def _references(shape_index, seed=5):
    """-> (layers, inputs, allocation of the phase-after-phase kernel, allocation of the three kernels); computed once per shape."""
    N, L3, K1, K2, K3, s3, p1, p2, p3, e1, e2, e3 = _shapes()[shape_index]
    c1, c2, c3 = layers = tc._front3_layers(N, L3, K1, K2, K3, s3, p1, p2, p3, 384, e1, e2, e3, os_t=384 + (0, 8)[L3 % 2])
    assert c3.Lout == L3
    t1 = tc._inputs(c1, seed=seed)
    b1 = c1.alloc_out(tc.dev())
    assert tc._call(c1, t1, b1.data_ptr() + 2 * cr.FRONT) == tc.K_FIRST
    t2 = tc._inputs(c2, seed=seed + 1, x=c1.out_view(b1)[c1.rows(tc.dev()).reshape(-1), :16].reshape(N, c1.Lout, 16).view(torch.float16))
    b2 = c2.alloc_out(tc.dev())
    tc._call(c2, t2, b2.data_ptr() + 2 * cr.FRONT)
    t3 = tc._inputs(c3, seed=seed + 2, x=c2.out_view(b2)[c2.rows(tc.dev()).reshape(-1), :16].reshape(N, c2.Lout, 16).view(torch.float16))
    three = c3.alloc_out(tc.dev())
    assert tc._call(c3, t3, three.data_ptr() + 2 * cr.FRONT) == tc.K_WS384
    t = (t1, t2, t3)
    phased = _fused(layers, t, dict(conv_front_pipe=0))
    assert bool((three != cr.SENTINEL).any())
    return layers, t, phased, three


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("shape_index", range(len(_shapes())), ids=[_sid(v) for v in _shapes()])
def test_pipeline_writes_the_bytes_of_both_references(shape_index, wgs):
    layers, t, phased, three = _references(shape_index)
    got = _fused(layers, t, dict(conv_front_pipe=1, conv_front_wgs=wgs))
    assert torch.equal(got, phased), "other bytes than the phase-after-phase fused kernel"
    assert torch.equal(got, three), "other bytes than conv3 of the three separate kernels"
    assert torch.equal(_fused(layers, t, dict(conv_front_pipe=1, conv_front_wgs=wgs)), got), "a second run wrote other bytes"


@pytest.mark.parametrize("wgs", (1, 2, 0))
def test_input_a_then_b_then_a(wgs):
    """A stale span buffer, conv1 slice or signal strip would show as bytes of B in the second run of A."""
    ia = len(_shapes()) - 2                                  # N = 3, L3 = 513, the hac layers
    layers, ta, phased, _ = _references(ia)
    lb, tb, phased_b, _ = _references(ia, seed=23)
    opts = dict(conv_front_pipe=1, conv_front_wgs=wgs)
    a1 = _fused(layers, ta, opts)
    b = _fused(lb, tb, opts)
    a2 = _fused(layers, ta, opts)
    assert torch.equal(b, phased_b) and not torch.equal(a1, b)
    assert torch.equal(a1, phased) and torch.equal(a2, a1)


def test_encoder_scores_are_the_same_bytes():
    """hac model, 5 chunks of 3100 samples (517 positions: blocks of 256, 256 and 5): the scores at the END of the encoder."""
    from bonito_amd import decode, synthetic
    from test_gpu_encoder import _encode
    model = synthetic.make_model("hac", batchsize=5, chunksize=3100)
    x = torch.randn(5, 1, 3100, generator=torch.Generator().manual_seed(31)).half().cuda()
    try:
        decode.set_option("conv_front_pipe", 0)
        phased, layout = _encode(model.encoder, x)
        decode.set_option("conv_front_pipe", 1)
        piped, _ = _encode(model.encoder, x)
        decode.set_option("conv_front_wgs", 2)               # two workgroups: runs of 7 and 8 blocks across the chunks
        piped2, _ = _encode(model.encoder, x)
    finally:
        tc._set(PIPE_DEFAULTS)
    assert "conv_front3_kernel" in layout and phased.shape[1] == 517
    assert torch.equal(piped, phased) and torch.equal(piped2, phased)
    assert torch.isfinite(phased.float()).all() and phased.float().abs().max().item() > 0.1
