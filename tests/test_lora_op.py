"""ops.lora_delta_add off the GPU: the eager expression, bit for bit."""

import torch
import torch.nn.functional as F


def test_cpu_path_is_the_eager_expression():
    from neuronx_distributed_training_amd.ops import lora_delta_add

    g = torch.Generator().manual_seed(0)
    shapes = ((2, 5, 16), (8, 16), (24, 8), (2, 5, 24))  # x, A, B, base
    grads = []
    for fn in (lora_delta_add,
               lambda base, x, A, B, s: base + F.linear(F.linear(x, A), B) * s):
        g.manual_seed(0)
        x, A, B, base = (torch.randn(s, generator=g).bfloat16()
                         .requires_grad_(True) for s in shapes)
        out = fn(base, x, A, B, 2.0)
        out.backward(torch.randn(out.shape, generator=g).bfloat16())
        grads.append((out.detach(), x.grad, A.grad, B.grad))
    for got, want in zip(*grads):
        assert torch.equal(got, want)
