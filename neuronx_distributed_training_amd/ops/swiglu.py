"""Fused SwiGLU (silu(gate) * up) — HIP kernel on GPU.

Replaces the reference's ActivationMultiplyMLP split/silu/mul
(modeling_llama.py:164-223): the fused gate_up ColumnParallel GEMM output
[..., 2*I/tp] is split in-kernel, saving one full activation round-trip
through HBM per MLP.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import bf16_kernels_for


def _ref_dtype(t: torch.Tensor) -> torch.dtype:
    # torch path (CPU, and GPU tensors that are not bf16): fp32 for
    # bf16/fp16/fp32 inputs, fp64 stays fp64
    return torch.promote_types(t.dtype, torch.float32)


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate_up: torch.Tensor):
        ctx.save_for_backward(gate_up)
        k = bf16_kernels_for(gate_up)
        if k is not None:
            return k.swiglu_fwd(gate_up.reshape(-1, gate_up.size(-1)).contiguous()).reshape(
                *gate_up.shape[:-1], gate_up.size(-1) // 2
            )
        gate, up = gate_up.chunk(2, dim=-1)
        return F.silu(gate.to(_ref_dtype(gate_up))).to(gate_up.dtype) * up

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        (gate_up,) = ctx.saved_tensors
        k = bf16_kernels_for(dy)
        if k is not None:
            d = k.swiglu_bwd(
                dy.reshape(-1, dy.size(-1)).contiguous(),
                gate_up.reshape(-1, gate_up.size(-1)).contiguous(),
            )
            return d.reshape(gate_up.shape)
        gate, up = gate_up.chunk(2, dim=-1)
        ct = _ref_dtype(gate_up)
        g = gate.to(ct)
        sig = torch.sigmoid(g)
        silu = g * sig
        dsilu = sig * (1 + g * (1 - sig))
        dyf = dy.to(ct)
        dgate = (dyf * up.to(ct) * dsilu).to(gate_up.dtype)
        dup = (dyf * silu).to(gate_up.dtype)
        return torch.cat((dgate, dup), dim=-1)


def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    """gate_up: [..., 2*I] laid out [gate | up]; returns [..., I]."""
    return _SwiGLUFn.apply(gate_up)
