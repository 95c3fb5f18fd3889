"""Fused LM-head + cross-entropy on the MI355X kernels (csrc/lm_head_loss.hip):
the per-token loss of ``hidden @ weight^T`` without the [N, V] logits.

forward:  (lmax, lsum, tgt) = lmhead_ce_fwd(hidden, weight, target)
          the TP reductions of the vocab-parallel loss (max, rescaled sum,
          target logit), loss = log(gsum) + gmax - tgt
          saved: hidden, weight, target, gmax, gsum -- nothing of size N * V
backward: per chunk of ``chunk_rows`` rows, into one reused [C, V] bf16 buffer
          dS = lmhead_ce_dlogits(...)       the tile is recomputed
          dH[chunk] = dS @ weight           library GEMM
          dW += dS^T @ hidden[chunk]        library GEMM, bf16 accumulator
          so dW is rounded to bf16 once per chunk, at most 8 times by default.

The kernels serve bf16 tensors on a GPU with H a multiple of the kernel's K
step (64), V a multiple of 8 and N > 0. ``parallel.loss.
parallel_linear_cross_entropy`` sends everything else to
``parallel_cross_entropy(F.linear(hidden, weight), target)``.
"""

from __future__ import annotations

import torch
import torch.distributed as dist

from ..parallel import state as ps
from . import require_extension

K_STEP = 64  # LMHEAD_BK of csrc/launch.h; the binding rejects any other H


def fused_path_supported(hidden: torch.Tensor, weight: torch.Tensor) -> bool:
    for t in (hidden, weight):
        if not t.is_cuda or t.dtype != torch.bfloat16:
            return False
    if weight.dim() != 2 or hidden.dim() < 1:
        return False
    V, H = weight.shape
    return (
        hidden.size(-1) == H
        and H > 0 and H % K_STEP == 0
        and V > 0 and V % 8 == 0
        and hidden.numel() > 0
    )


def default_chunk_rows(n: int, tile: int) -> int:
    """ceil(n / 8) rounded up to the token tile: at most 8 chunks."""
    per_chunk = -(-n // 8)
    return max(-(-per_chunk // tile), 1) * tile


class _LinearCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, weight, target, chunk_rows):
        k = require_extension()
        tp = ps.get_tensor_model_parallel_world_size()
        group = ps.get_tensor_model_parallel_group()
        vocab_start = ps.get_tensor_model_parallel_rank() * weight.size(0)
        hidden, weight = hidden.contiguous(), weight.contiguous()
        target = target.contiguous()
        lmax, lsum, tgt = k.lmhead_ce_fwd(hidden, weight, target, vocab_start)
        if tp > 1:
            gmax = lmax.clone()
            dist.all_reduce(gmax, op=dist.ReduceOp.MAX, group=group)
            gsum = lsum * torch.exp(lmax - gmax)
            dist.all_reduce(gsum, group=group)
            dist.all_reduce(tgt, group=group)
        else:
            gmax, gsum = lmax, lsum
        ctx.save_for_backward(hidden, weight, target, gmax, gsum)
        ctx.vocab_start = vocab_start
        ctx.chunk_rows = chunk_rows or default_chunk_rows(
            hidden.size(0), k.LMHEAD_BM)
        return gsum.log() + gmax - tgt

    @staticmethod
    def backward(ctx, grad_out):
        k = require_extension()
        hidden, weight, target, gmax, gsum = ctx.saved_tensors
        N, C = hidden.size(0), min(ctx.chunk_rows, hidden.size(0))
        gout = grad_out.float().contiguous()
        need_h, need_w = ctx.needs_input_grad[:2]
        ds_buf = torch.empty(C, weight.size(0), dtype=hidden.dtype,
                             device=hidden.device)
        dh = torch.empty_like(hidden) if need_h else None
        dw = torch.empty_like(weight) if need_w else None
        for r0 in range(0, N, C):
            rows = min(C, N - r0)
            k.lmhead_ce_dlogits(hidden, weight, target, gmax, gsum, gout,
                                ctx.vocab_start, r0, rows, ds_buf)
            ds = ds_buf[:rows]
            if need_h:
                torch.mm(ds, weight, out=dh[r0:r0 + rows])
            if need_w and r0 == 0:
                torch.mm(ds.t(), hidden[:rows], out=dw)
            elif need_w:
                dw.addmm_(ds.t(), hidden[r0:r0 + rows])
        return dh, dw, None, None


def linear_cross_entropy(hidden: torch.Tensor, weight: torch.Tensor,
                         target: torch.Tensor, chunk_rows=None) -> torch.Tensor:
    """Per-token loss [N] of hidden [N, H] @ weight [V, H]^T (this TP rank's
    vocab shard) against target [N] global ids, on the fused kernels only:
    inputs they do not serve are an error here (see fused_path_supported)."""
    if not fused_path_supported(hidden, weight) or hidden.dim() != 2:
        raise ValueError(
            "linear_cross_entropy needs bf16 GPU tensors hidden [N, H] and "
            f"weight [V, H] with N > 0, H % {K_STEP} == 0 and V % 8 == 0; got "
            f"{tuple(hidden.shape)} {hidden.dtype} and {tuple(weight.shape)} "
            f"{weight.dtype} on {hidden.device}"
        )
    if chunk_rows is not None and chunk_rows <= 0:
        raise ValueError(f"chunk_rows must be positive, got {chunk_rows}")
    return _LinearCrossEntropy.apply(hidden, weight, target, chunk_rows)
