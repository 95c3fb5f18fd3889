"""ops.layernorm / gelu / geglu off the kernels: on the CPU they are the torch
expressions they replace, bit for bit, forward and gradients."""

import pytest
import torch
import torch.nn.functional as F

from neuronx_distributed_training_amd import ops
from neuronx_distributed_training_amd.ops.layernorm import LayerNorm


def _grads(fn, *inputs, dy):
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    y = fn(*leaves)
    return (y.detach(), *torch.autograd.grad(y, leaves, dy))


def _geglu_torch(gu):
    g, u = gu.chunk(2, dim=-1)
    return F.gelu(g) * u


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_paths_are_torch(dtype):
    g = torch.Generator().manual_seed(5)
    x, dy = (torch.randn(3, 7, 40, generator=g).to(dtype) for _ in range(2))
    gu = torch.randn(3, 7, 80, generator=g).to(dtype)
    w, b = (torch.randn(40, generator=g).to(dtype) for _ in range(2))
    for ours, theirs, inputs in (
        (lambda x, w, b: ops.layernorm(x, w, b, 1e-6),
         lambda x, w, b: F.layer_norm(x, (40,), w, b, 1e-6), (x, w, b)),
        (ops.gelu, F.gelu, (x,)),
        (ops.geglu, _geglu_torch, (gu,)),
    ):
        for a, t in zip(_grads(ours, *inputs, dy=dy),
                        _grads(theirs, *inputs, dy=dy)):
            assert a.dtype == t.dtype and torch.equal(a, t)


def test_layernorm_module_and_switch(monkeypatch):
    m = LayerNorm(16, 1e-6)
    assert isinstance(m, torch.nn.LayerNorm)
    assert list(m.state_dict()) == ["weight", "bias"]
    x = torch.randn(2, 16)
    want = torch.nn.LayerNorm.forward(m, x)
    for arm in ("1", "0"):
        monkeypatch.setenv("NXDT_GPT_GLUE", arm)
        assert torch.equal(m(x), want)
    monkeypatch.setenv("NXDT_GPT_GLUE", "yes")
    with pytest.raises(ValueError):
        m(x)
    with pytest.raises(ValueError):
        ops.gpt_glue()
