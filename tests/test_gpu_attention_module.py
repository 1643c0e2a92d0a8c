"""bonito_amd.attn.mha_module on the device (-m gpu): a MultiHeadAttention container as Wqkv -> rotary + windowed attention -> out_proj,
differentiable, with gradients on the container's fp32 parameters.

exact = the reference's MultiHeadAttention.forward restated in fp64 torch with autograd; yardstick = the same restatement run by torch in
fp16 on the CPU (tests/attention_train_ref.py, pinned by tests/test_attention_train_ref_cpu.py). With dist(a) = max|a - exact| / max|exact|,
each of y, dx, dWqkv, dWo, dbo (and dbqkv of a qkv_bias container) must satisfy dist(kernel) <= 2 dist(yardstick): the project's margin for
composed training layers (tests/test_gpu_lstm_train.py, tests/test_gpu_train_layers.py). Every case prints its ratios; DESIGN.md section 6
records them."""
import functools

import pytest
import torch

import attention_train_ref as tr
from bonito_amd import attn
from bonito_amd.transformer.model import MultiHeadAttention

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 2.0
SHAPES = ((2, 40, (3, 5)), (1, 150, (40, 41)), (1, 300, (127, 128)))      # (N, T, window)


@functools.lru_cache(maxsize=None)
def _references(N, T, D, H, window, qkv_bias):
    """(case, exact, yardstick), computed once on the CPU and never modified."""
    case = tr.make_mha_case(N, T, D, qkv_bias, seed=1)
    return case, tr.mha_exact(case, H, window), tr.mha_yardstick(case, H, window)


def _container(case, D, H, window, qkv_bias):
    layer = MultiHeadAttention(D, H, qkv_bias=qkv_bias, attn_window=window)
    with torch.no_grad():
        layer.Wqkv.weight.copy_(case["wqkv"])
        layer.out_proj.weight.copy_(case["wo"])
        layer.out_proj.bias.copy_(case["bo"])
        if qkv_bias:
            layer.Wqkv.bias.copy_(case["bqkv"])
    return layer.to(DEV)


def _run(N, T, D, H, window, qkv_bias):
    case, exact, yard = _references(N, T, D, H, window, qkv_bias)
    layer = _container(case, D, H, window, qkv_bias)
    x = case["x"].to(DEV).requires_grad_()
    y = attn.mha_module(layer, x)
    assert y.dtype == torch.float16 and tuple(y.shape) == (N, T, D)
    y.backward(case["dy"].to(DEV))
    torch.cuda.synchronize()
    params = (layer.Wqkv.weight, layer.Wqkv.bias, layer.out_proj.weight, layer.out_proj.bias)
    for p in params:
        assert p is None or (p.dtype == torch.float32 and p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape)
    assert x.grad.dtype == torch.float16
    got = (y.detach(), x.grad) + tuple(None if p is None else p.grad for p in params)
    failed = []
    for name, g, e, yd in zip(tr.MHA_NAMES, got, exact, yard):
        if e is None:
            assert g is None and name == "dbqkv" and not qkv_bias
            continue
        dk, dy = tr.dist(g.cpu().numpy(), e.numpy()), tr.dist(yd.numpy(), e.numpy())
        print("mha N=%d T=%d D=%d H=%d %s%s %-6s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f"
              % (N, T, D, H, window, " qkv_bias" if qkv_bias else "", name, dk, dy, dk / dy if dy > 0 else float("inf")))
        if not dk <= MARGIN * dy:
            failed.append((name, dk, dy))
    assert not failed, failed


@pytest.mark.parametrize("N,T,window", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("D,H", [(128, 2), (192, 3)])
def test_module_within_twice_the_yardstick(D, H, N, T, window):
    _run(N, T, D, H, window, qkv_bias=False)


def test_module_with_a_qkv_bias():
    _run(2, 40, 128, 2, (3, 5), qkv_bias=True)


def test_gradients_accumulate_on_the_container_and_fp32_input_gets_fp32_gradient():
    N, T, D, H, window = 2, 40, 128, 2, (3, 5)
    case, _, _ = _references(N, T, D, H, window, False)
    layer = _container(case, D, H, window, False)
    x = case["x"].to(DEV).float().requires_grad_()
    dy = case["dy"].to(DEV)
    attn.mha_module(layer, x).backward(dy)
    assert x.grad.dtype == torch.float32
    once = layer.Wqkv.weight.grad.clone()
    attn.mha_module(layer, x).backward(dy)
    assert torch.equal(layer.Wqkv.weight.grad, 2 * once)                     # the same bytes twice, added by autograd
    assert layer.Wqkv.bias is None
