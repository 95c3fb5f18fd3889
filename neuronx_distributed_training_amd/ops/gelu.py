"""Exact (erf) GELU and GEGLU (gelu(gate) * up) with HIP kernels on GPU.

The Megatron GPT family's ``activation: gelu | geglu`` (reference
transformer.py ParallelMLP). bf16 GPU tensors take ops/csrc/gelu.hip: one
HBM pass each way; GEGLU splits the fused gate_up ColumnParallel output
[..., 2*I/tp] inside the kernel and its backward writes [dgate | dup] in
place, with no chunk views and no cat. Everything else (CPU, GPU tensors of
another dtype) is the torch expression itself under plain autograd:
``F.gelu(h)``, and ``F.gelu(g) * u`` on the chunk views.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import bf16_kernels_for


def _rows(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(-1, t.size(-1)).contiguous()


class _GELUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return bf16_kernels_for(x).gelu_fwd(_rows(x)).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return bf16_kernels_for(x).gelu_bwd(_rows(dy), _rows(x)).view(x.shape)


class _GEGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate_up):
        ctx.save_for_backward(gate_up)
        y = bf16_kernels_for(gate_up).geglu_fwd(_rows(gate_up))
        return y.view(*gate_up.shape[:-1], gate_up.size(-1) // 2)

    @staticmethod
    def backward(ctx, dy):
        (gate_up,) = ctx.saved_tensors
        d = bf16_kernels_for(gate_up).geglu_bwd(_rows(dy), _rows(gate_up))
        return d.view(gate_up.shape)


def gelu(x: torch.Tensor) -> torch.Tensor:
    """Exact GELU. bf16 GPU tensors always take the HIP kernels (last
    dimension divisible by 8)."""
    if bf16_kernels_for(x) is None:
        return F.gelu(x)
    return _GELUFn.apply(x)


def geglu(gate_up: torch.Tensor) -> torch.Tensor:
    """gate_up: [..., 2*I] laid out [gate | up]; returns gelu(gate) * up,
    [..., I]. bf16 GPU tensors always take the HIP kernels (I divisible by
    8)."""
    if bf16_kernels_for(gate_up) is None:
        gate, up = gate_up.chunk(2, dim=-1)
        return F.gelu(gate) * up
    return _GEGLUFn.apply(gate_up)
