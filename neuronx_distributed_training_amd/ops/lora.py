"""LoRA adapter delta on the MI355X skinny-GEMM kernels (csrc/lora.hip).

    out = base_out + scaling * (x @ A^T) @ B^T

forward:  h = shrink(x, A)                  [T, r], bf16
          out = expand(h, B, scaling, base) one read of base, one write
backward: d_base = dout                     (the same tensor, no copy)
          dh = shrink(dout, B^T, scaling)   [T, r], bf16
          dx = expand(dh, A^T)
          dA = wgrad(x, dh)                 [r, K], lora_A's layout
          dB = wgrad(dout, h, scaling)      [N, r], lora_B's layout

The kernels serve bf16 tensors on a GPU with r in {8, 16, 32, 64} and K, N
multiples of 8. Everything else (CPU, fp32 or autocast modules, other ranks
or alignments) evaluates the eager expression under plain autograd, bit for
bit what the module computed before this op existed. NXDT_LORA_FUSED=0 (read
per call) forces the eager expression on a GPU too, for A/B runs.
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import require_extension

RANKS = (8, 16, 32, 64)


def _eager(base_out, x, lora_A, lora_B, scaling):
    return base_out + F.linear(F.linear(x, lora_A), lora_B) * scaling


def fused_path_supported(base_out, x, lora_A, lora_B) -> bool:
    for t in (base_out, x, lora_A, lora_B):
        if not t.is_cuda or t.dtype != torch.bfloat16:
            return False
    if lora_A.dim() != 2 or lora_B.dim() != 2 or x.dim() < 1:
        return False
    r, K = lora_A.shape
    N = lora_B.size(0)
    return (
        r in RANKS
        and lora_B.size(1) == r
        and K > 0 and K % 8 == 0
        and N > 0 and N % 8 == 0
        and x.size(-1) == K
        and base_out.shape == x.shape[:-1] + (N,)
    )


class _LoraDeltaAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, base_out, x, lora_A, lora_B, scaling):
        k = require_extension()
        K, N = lora_A.size(1), lora_B.size(0)
        x2 = x.reshape(-1, K).contiguous()
        h = k.lora_shrink(x2, lora_A.contiguous(), 1.0)
        out = k.lora_expand(h, lora_B.contiguous(), scaling,
                            base_out.reshape(-1, N).contiguous())
        ctx.save_for_backward(x2, h, lora_A, lora_B)
        ctx.scaling = scaling
        ctx.x_shape = x.shape
        return out.view(base_out.shape)

    @staticmethod
    def backward(ctx, dout):
        x2, h, lora_A, lora_B = ctx.saved_tensors
        k = require_extension()
        d2 = dout.reshape(-1, lora_B.size(0)).contiguous()
        # the [r, N] / [K, r] transposed copies are r * (N + K) elements
        dh = k.lora_shrink(d2, lora_B.t().contiguous(), ctx.scaling)
        dx = None
        if ctx.needs_input_grad[1]:
            dx = k.lora_expand(dh, lora_A.t().contiguous(), 1.0, None)
            dx = dx.view(ctx.x_shape)
        dA = k.lora_wgrad(x2, dh, 1.0, True)
        dB = k.lora_wgrad(d2, h, ctx.scaling, False)
        return dout, dx, dA, dB, None


def lora_delta_add(base_out: torch.Tensor, x: torch.Tensor,
                   lora_A: torch.Tensor, lora_B: torch.Tensor,
                   scaling: float) -> torch.Tensor:
    """base_out [..., N] + scaling * (x [..., K] @ lora_A [r, K]^T) @
    lora_B [N, r]^T; the leading dimensions are flattened to T."""
    if (os.environ.get("NXDT_LORA_FUSED", "") != "0"
            and fused_path_supported(base_out, x, lora_A, lora_B)):
        return _LoraDeltaAdd.apply(base_out, x, lora_A, lora_B,
                                   float(scaling))
    return _eager(base_out, x, lora_A, lora_B, scaling)
