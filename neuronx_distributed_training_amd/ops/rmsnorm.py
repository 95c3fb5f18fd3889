"""RMSNorm with a hand-written CDNA4 HIP kernel on GPU.

Replaces the reference's ``modules.rms_norm.RMSNorm`` / apex
``MixedFusedRMSNorm`` (reference fused_layer_norm.py:18-36,
modeling_llama.py:145-161). Forward computes y = x * w / rms(x) in one
HBM pass (fp32 accumulation, bf16 IO, vectorized bf16x8 loads); backward
fuses dx and a two-stage dw reduction.
"""

from __future__ import annotations

import torch

from . import bf16_kernels_for


def _kernel_weight(weight: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """The kernels read the weight as bf16 (the binding rejects anything
    else). A weight kept in another dtype — RMSNorm's default is fp32, and
    "autocast" precision keeps fp32 parameters — is cast to the activation
    dtype for the kernel; its gradient is returned in its own dtype."""
    return weight if weight.dtype == x.dtype else weight.to(x.dtype)


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, eps: float):
        k = bf16_kernels_for(x)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        if k is not None:
            y, invrms = k.rmsnorm_fwd(
                x2.contiguous(), _kernel_weight(weight, x2), eps
            )
        else:
            xf = x2.float()
            invrms = torch.rsqrt(xf.pow(2).mean(-1) + eps)
            y = (xf * invrms.unsqueeze(-1) * weight.float()).to(x.dtype)
        ctx.save_for_backward(x2, weight, invrms)
        ctx.eps = eps
        return y.reshape(shp)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x2, weight, invrms = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        k = bf16_kernels_for(dy2)
        if k is not None:
            dx, dw = k.rmsnorm_bwd(
                dy2, x2.contiguous(), _kernel_weight(weight, x2), invrms
            )
            # the kernel's fp32 sum, rounded once, to the weight's own dtype
            dw = dw.to(weight.dtype)
        else:
            xf = x2.float()
            dyf = dy2.float()
            wf = weight.float()
            r = invrms.unsqueeze(-1)
            xhat = xf * r
            wdy = dyf * wf
            # dx = r*(wdy - xhat * mean(wdy*xhat))
            c = (wdy * xhat).mean(-1, keepdim=True)
            dx = (r * (wdy - xhat * c)).to(dy.dtype)
            dw = (dyf * xhat).sum(0).to(weight.dtype)
        return dx.reshape(dy.shape), dw, None


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    return _RMSNormFn.apply(x, weight, eps)


class RMSNorm(torch.nn.Module):
    def __init__(self, hidden_size: int, eps: float = 1e-5, dtype: torch.dtype = torch.float32):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(hidden_size, dtype=dtype))
        self.variance_epsilon = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return rmsnorm(x, self.weight, self.variance_epsilon)

    def extra_repr(self):
        return f"{self.weight.numel()}, eps={self.variance_epsilon}"
