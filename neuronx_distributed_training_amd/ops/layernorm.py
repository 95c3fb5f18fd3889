"""LayerNorm with hand-written CDNA4 HIP kernels on GPU.

The Megatron GPT family's ``normalization: layernorm`` (reference
transformer.py get_layer_norm / apex MixedFusedLayerNorm). bf16 GPU tensors
take ``layernorm_fwd`` / ``layernorm_bwd`` (ops/csrc/layernorm.hip): a wave
per row up to H = 2048, a block per row beyond, fp32 statistics from
register-held values, and a two-stage atomic-free sum for the weight and
bias gradients, bit-reproducible from run to run. Everything else (CPU, GPU
tensors of another dtype) is ``F.layer_norm`` itself under plain autograd.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import bf16_kernels_for


def _kernel_param(p: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """The kernels read weight and bias as bf16. A parameter kept in another
    dtype ("autocast" precision keeps fp32 parameters) is cast for the
    kernel; its gradient is returned in its own dtype."""
    return p if p.dtype == x.dtype else p.to(x.dtype)


class _LayerNormFn(torch.autograd.Function):
    """bf16 GPU tensors only (layernorm() dispatches)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        k = bf16_kernels_for(x)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        y, mean, rstd = k.layernorm_fwd(
            x2, _kernel_param(weight, x2), _kernel_param(bias, x2), eps
        )
        ctx.save_for_backward(x2, weight, bias, mean, rstd)
        return y.view(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias, mean, rstd = ctx.saved_tensors
        k = bf16_kernels_for(x2)
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx, dw, db = k.layernorm_bwd(
            dy2, x2, _kernel_param(weight, x2), mean, rstd
        )
        # the kernels' fp32 sums, rounded once, to each parameter's own dtype
        return (dx.view(dy.shape), dw.to(weight.dtype), db.to(bias.dtype),
                None)


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              eps: float = 1e-5) -> torch.Tensor:
    """LayerNorm over the last dimension with torch's definition (biased
    variance). bf16 GPU tensors always take the HIP kernels, which need both
    weight and bias and a last dimension divisible by 8."""
    if bf16_kernels_for(x) is None:
        return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    if weight is None or bias is None:
        raise ValueError("the LayerNorm kernels need a weight and a bias")
    return _LayerNormFn.apply(x, weight, bias, eps)


class LayerNorm(torch.nn.LayerNorm):
    """nn.LayerNorm (same parameters, same state-dict keys ``weight`` and
    ``bias``; found by every isinstance check for nn.LayerNorm, such as
    parallel.layers.tag_sequence_parallel_params) whose forward runs the HIP
    kernels. NXDT_GPT_GLUE=0 makes it nn.LayerNorm's own forward, for A/B."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from . import gpt_glue

        if not gpt_glue() or len(self.normalized_shape) != 1:
            return super().forward(x)
        return layernorm(x, self.weight, self.bias, self.eps)
