"""Split-KV flash decode: attention of a short query step over a
preallocated KV cache, read in place (``csrc/flash_attn_decode.hip``).

``q`` is ``[B, HQ, S_q, D]``; ``k`` / ``v`` are cache buffers
``[B, HKV, CAP, D]`` (``d`` contiguous, any other strides). Batch row ``b``
sees keys ``kv_lo[b] <= j < kv_hi[b]``; query ``i`` sits at position
``p = kv_hi[b] - S_q + i`` (bottom-right causal) and sees ``j <= p``, and
``j > p - window`` with a sliding window. Whatever the buffers hold outside
``[kv_lo[b], kv_hi[b])`` is never used and may be NaN. A row with no alive
key gives ``O = 0`` and ``LSE = -1e30``, like the ranged kernels.

Forward only: there is no backward kernel and no autograd node.

GPU: bf16, head_dim 64 / 128, ``(HQ / HKV) * S_q <= 64``; one block serves
all query heads of a kv head for one slice of the keys, and a second kernel
merges the slices. The number of slices comes from ``B``, ``HKV``,
``max_kv`` and the CU count, never from the device lengths, so a call makes
no host sync. CPU: an fp32 torch reference with the same semantics.
"""

from __future__ import annotations

import math

import torch

from . import kernels_for
from .flash_attn import _ranged_softmax


def _cpu_ref_decode(q, k, v, kv_lo, kv_hi, max_kv, scale, window):
    b, hq, sq, _ = q.shape
    g = hq // k.size(1)
    hi = kv_hi.long().clamp(0, max_kv)
    lo = torch.minimum(kv_lo.long().clamp(0, max_kv), hi)
    j = torch.arange(max_kv, device=q.device)
    in_range = (j[None] >= lo[:, None]) & (j[None] < hi[:, None])  # [b, kv]
    # out-of-range cache content is garbage: select it away before any
    # arithmetic (0 * NaN would survive a zero probability)
    keep = in_range[:, None, :, None]
    zero = torch.zeros((), dtype=torch.float32, device=q.device)
    kf = torch.where(keep, k[:, :, :max_kv].float(), zero)
    vf = torch.where(keep, v[:, :, :max_kv].float(), zero)
    kf = kf.repeat_interleave(g, dim=1)
    vf = vf.repeat_interleave(g, dim=1)
    p = hi[:, None] - sq + torch.arange(sq, device=q.device)[None]  # [b, sq]
    dead = ~in_range[:, None, :] | (j[None, None] > p[:, :, None])
    if window > 0:
        dead |= j[None, None] <= (p[:, :, None] - window)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) * scale
    prob, lse = _ranged_softmax(s, dead[:, None])
    return torch.matmul(prob, vf).to(q.dtype), lse


def flash_attn_decode(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    kv_hi: torch.Tensor,
    kv_lo: torch.Tensor | None = None,
    *,
    max_kv: int | None = None,
    scale: float | None = None,
    window: int | None = None,
    num_splits: int | None = None,
    return_lse: bool = False,
):
    """kv_hi / kv_lo: int tensors [B] on q's device (kv_lo None = zeros).

    max_kv: host int with ``kv_hi[b] <= max_kv <= CAP``; only keys below it
    are visited. None = CAP. Values of kv_hi above it are clamped.

    num_splits: number of key slices; None lets the host heuristic choose.
    For a given value the result is bit-reproducible. Ignored on CPU.

    Returns ``O`` ``[B, HQ, S_q, D]`` in q's dtype, and with ``return_lse``
    also ``LSE`` ``[B, HQ, S_q]`` fp32. Forward only: inputs that require
    grad while autograd is enabled raise."""
    if torch.is_grad_enabled() and (
        q.requires_grad or k.requires_grad or v.requires_grad
    ):
        raise RuntimeError(
            "flash_attn_decode is forward only: call it under "
            "torch.no_grad() or use flash_attn_func"
        )
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape:
        raise ValueError(
            "flash_attn_decode: q must be [B, HQ, S_q, D] and k / v "
            f"[B, HKV, CAP, D], got {tuple(q.shape)}, {tuple(k.shape)}, "
            f"{tuple(v.shape)}"
        )
    b, hq, sq, d = q.shape
    cap = k.size(2)
    if k.size(0) != b or k.size(3) != d or k.size(1) == 0 \
            or hq % k.size(1) != 0:
        raise ValueError(
            f"flash_attn_decode: k / v {tuple(k.shape)} do not match q "
            f"{tuple(q.shape)}"
        )
    max_kv = cap if max_kv is None else int(max_kv)
    if not 1 <= max_kv <= cap:
        raise ValueError(f"max_kv {max_kv} must be in [1, CAP = {cap}]")
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    window = int(window or 0)
    kv_hi = torch.as_tensor(kv_hi, device=q.device).to(torch.int32)
    kv_hi = kv_hi.reshape(-1).contiguous()
    if kv_lo is None:
        kv_lo = torch.zeros_like(kv_hi)
    kv_lo = torch.as_tensor(kv_lo, device=q.device).to(torch.int32)
    kv_lo = kv_lo.reshape(-1).contiguous()
    if kv_hi.numel() != b or kv_lo.numel() != b:
        raise ValueError(f"kv_lo / kv_hi must have shape [{b}]")
    kern = kernels_for(q)
    if kern is not None:
        o, lse = kern.flash_attn_decode(
            q, k, v, kv_lo, kv_hi, max_kv, float(scale), window,
            int(num_splits or 0),
        )
    else:
        o, lse = _cpu_ref_decode(q, k, v, kv_lo, kv_hi, max_kv, float(scale),
                                 window)
    return (o, lse) if return_lse else o
