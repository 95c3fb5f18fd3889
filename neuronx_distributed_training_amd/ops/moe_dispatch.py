"""Fused MoE token path on the MI355X (ops/csrc/moe_dispatch.hip).

From the router's ``(topw, topi)`` to the layer output through the grouped
expert GEMMs, with no torch indexing op and no token-sorted intermediate:

    plan     counting sort of the T*k (token, choice) pairs by expert, written
             straight into the 256-row-aligned padded layout of ``moe_gemm``
             (three launches, no global atomics, no host sync);
    permute  x_pad[r] = x[row_src[r] // k], zeros in a segment's padding rows;
    experts  ``moe_gemm.padded_expert_mlp`` (gate_up GEMM, SwiGLU, down GEMM);
    combine  y[t] = sum_j topw[t, j] * y_pad[slot[t, j]], fp32 over the k rows,
             one rounding to bf16; capacity-dropped pairs (slot -1) skipped.

The backward is the same kernels the other way round: the combine's backward
writes dy_pad and d topw from one read of dy and y_pad, the permute's backward
is the combine with unit weights.

Rounding points that differ from the eager layer (modules/moe.py): eager
rounds ``yexp * w`` to bf16 and sums the k rows in bf16 with atomics, in the
backward it rounds ``dy * yexp`` to bf16 before the sum over H, and it sums
the k rows of dx in bf16; here each of the three is one fp32 sum with one
rounding, in a fixed order (two runs are bit-equal).
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from . import require_extension
from .moe_gemm import padded_expert_mlp

MAX_EXPERTS = 64   # MOE_PLAN_MAX_E: one wave lane per expert in the plan
MAX_TOP_K = 8      # MOE_MAX_TOPK: slots a combine lane keeps in registers


class MoEPlan(NamedTuple):
    """Device tensors of one routing decision. counts int64 [E] kept pairs per
    expert; pad_off int32 [E+1], total int32 [1] and tile_expert int32
    [Tp/256] as ``moe_gemm._layout`` gives them; slot int32 [T, k] the padded
    row of each pair (-1: dropped by the capacity); row_src int32 [Tp] the
    pair of each valid padded row (padding rows are not filled)."""
    counts: torch.Tensor
    pad_off: torch.Tensor
    total: torch.Tensor
    tile_expert: torch.Tensor
    slot: torch.Tensor
    row_src: torch.Tensor


def moe_plan(topi: torch.Tensor, num_experts: int, capacity: int = 0) -> MoEPlan:
    """topi: [T, k] int64 expert ids as ``topk`` returns them. capacity: most
    pairs an expert keeps, in ascending pair order (0: dropless)."""
    c, pad_off, total, tile_e, slot, row_src = require_extension().moe_plan(
        topi, num_experts, capacity)
    return MoEPlan(c, pad_off, total, tile_e, slot.view(topi.shape), row_src)


def _rows(plan: MoEPlan):
    return (plan.row_src, plan.tile_expert, plan.pad_off, plan.counts,
            plan.total)


class _Permute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        ctx.save_for_backward(plan.slot)
        return require_extension().moe_permute(x, plan.slot.size(1),
                                               *_rows(plan))

    @staticmethod
    def backward(ctx, dx_pad):
        (slot,) = ctx.saved_tensors
        return require_extension().moe_combine(dx_pad.contiguous(), slot), None


class _Combine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_pad, w, plan):
        ctx.save_for_backward(y_pad, w, plan.slot, *_rows(plan))
        return require_extension().moe_combine(y_pad, plan.slot, w)

    @staticmethod
    def backward(ctx, dy):
        y_pad, w, slot, *rows = ctx.saved_tensors
        dy_pad, dw = require_extension().moe_combine_bwd(
            dy.contiguous(), y_pad, w, slot, *rows)
        return dy_pad, dw, None


def moe_permute(x: torch.Tensor, plan: MoEPlan) -> torch.Tensor:
    """x: [T, H] bf16 -> x_pad [Tp, H]; rows at or past plan.total are left
    unwritten."""
    return _Permute.apply(x, plan)


def moe_combine(y_pad: torch.Tensor, w: torch.Tensor, plan: MoEPlan):
    """y_pad: [Tp, H] bf16, w: [T, k] bf16 or fp32 -> y [T, H] bf16."""
    return _Combine.apply(y_pad, w, plan)


def fused_moe_experts(x: torch.Tensor, topw: torch.Tensor, topi: torch.Tensor,
                      gate_up: torch.Tensor, down: torch.Tensor,
                      capacity: int = 0) -> torch.Tensor:
    """x: [T, H] bf16 on the GPU; topw, topi: [T, k] router weights and
    expert ids; gate_up: [E, 2I, H]; down: [E, H, I]. Returns
    y[t] = sum_j topw[t, j] * MLP_{topi[t, j]}(x[t]) over the pairs the
    capacity keeps. There is no other path: CPU tensors raise."""
    E, k = gate_up.size(0), topi.size(1)
    if E > MAX_EXPERTS or k > MAX_TOP_K:
        raise ValueError(f"fused_moe_experts: at most {MAX_EXPERTS} experts "
                         f"and top-{MAX_TOP_K}, got {E} and top-{k}")
    plan = moe_plan(topi.contiguous(), E, capacity)
    x_pad = moe_permute(x, plan)
    y_pad = padded_expert_mlp(x_pad, plan.tile_expert, plan.pad_off,
                              plan.total, gate_up, down)
    return moe_combine(y_pad, topw.contiguous(), plan)
