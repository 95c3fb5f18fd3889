"""Mixture-of-experts stack for MI355X.

Capability parity with the reference's NxD MoE
(``modules.moe.{model.MoE, expert_mlps.ExpertMLPs, routing.RouterTopK/
RouterSinkhorn, loss_function.load_balancing_loss_func}``; call sites
transformer.py:423-464, modeling_mixtral.py:342-374 — SURVEY.md §2.3):

- RouterTopK (softmax→top-k) and RouterSinkhorn (sinkhorn iterations);
- dropless expert compute (sort tokens by expert, one hipBLASLt GEMM per
  local expert) and capacity-factor mode (drop overflow tokens);
- expert parallelism: all-to-all token dispatch over the EP group
  (RCCL over xGMI), experts sharded across EP ranks;
- load-balancing auxiliary loss.

Expert MLPs are SwiGLU (gate_up fused + down), matching the dense path.
"""

from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from ..parallel import state as ps
from ..ops import swiglu

__all__ = ["RouterTopK", "RouterSinkhorn", "ExpertMLPs", "MoE",
           "load_balancing_loss_func", "token_shuffle", "token_unshuffle"]


class _AllToAll(torch.autograd.Function):
    """Autograd-aware variable-split all-to-all over the EP group."""

    @staticmethod
    def forward(ctx, x, out_splits, in_splits, group):
        ctx.out_splits = out_splits
        ctx.in_splits = in_splits
        ctx.group = group
        out = x.new_empty(int(sum(out_splits)), *x.shape[1:])
        dist.all_to_all_single(out, x, out_splits, in_splits, group=group)
        return out

    @staticmethod
    def backward(ctx, grad):
        out = grad.new_empty(int(sum(ctx.in_splits)), *grad.shape[1:])
        dist.all_to_all_single(
            out, grad.contiguous(), ctx.in_splits, ctx.out_splits, group=ctx.group
        )
        return out, None, None, None


# shared call counter so every rank in a shuffle group derives the same
# permutation seed without communication (layers step in lockstep).
_SHUFFLE_CALLS = 0


def _route_tokens(x: torch.Tensor, slots_all: torch.Tensor, group, r: int):
    """Move token i of rank src to global slot slots_all[src, i] within the
    shuffle group (slot g*T..(g+1)*T-1 lives on rank g). slots_all is a
    permutation of range(g*T), identical on every rank. Differentiable."""
    g, T = slots_all.shape
    slots = slots_all[r]
    dest = torch.div(slots, T, rounding_mode="floor")
    order = torch.argsort(dest, stable=True)
    in_splits = torch.bincount(dest, minlength=g).tolist()
    dest_all = torch.div(slots_all, T, rounding_mode="floor")
    out_splits = [(dest_all[src] == r).sum().item() for src in range(g)]
    recv = _AllToAll.apply(
        x[order.to(x.device)].contiguous(), out_splits, in_splits, group
    )
    # received rows arrive grouped by src rank, original-order within src;
    # place each at its target in-slab position.
    recv_slots = torch.cat([slots_all[src][dest_all[src] == r] for src in range(g)])
    pos = recv_slots - r * T
    inv = torch.empty(T, dtype=torch.long)
    inv[pos] = torch.arange(T)
    return recv[inv.to(x.device)]


def token_shuffle(x: torch.Tensor, group_size: int):
    """Randomly permute tokens across `group_size` adjacent DP ranks before
    MoE routing so capacity-mode load is balanced across the group
    (reference transformer.py:463 / megatron_gpt_model.py:134
    ``token_shuffle_group_size``). Returns (shuffled_x, ctx); pass ctx to
    ``token_unshuffle`` to restore order. x: [T, H], same T on every rank."""
    global _SHUFFLE_CALLS
    _SHUFFLE_CALLS += 1
    if group_size <= 1 or not dist.is_initialized():
        return x, None
    group, r = ps.get_token_shuffle_group(group_size)
    T = x.size(0)
    gen = torch.Generator().manual_seed(0x51F0 + _SHUFFLE_CALLS)
    perm = torch.randperm(group_size * T, generator=gen)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(group_size * T)
    y = _route_tokens(x, inv.view(group_size, T), group, r)
    return y, (perm.view(group_size, T), group, r)


def token_unshuffle(y: torch.Tensor, ctx):
    """Inverse of ``token_shuffle`` (returns tokens to their home rank and
    original order)."""
    if ctx is None:
        return y
    perm, group, r = ctx
    return _route_tokens(y, perm, group, r)


# backward scale for attached aux losses: the PP engine divides the main
# loss by num_microbatches before backward, so attached aux grads must
# carry the same factor (Megatron MoEAuxLossAutoScaler.set_loss_scale)
_AUX_LOSS_SCALE = 1.0


def set_aux_loss_scale(scale: float):
    global _AUX_LOSS_SCALE
    _AUX_LOSS_SCALE = float(scale)


class _AttachAuxLoss(torch.autograd.Function):
    """Route an auxiliary scalar's gradient through the activation chain
    (Megatron MoEAuxLossAutoScaler pattern): forward passes x through
    unchanged; backward hands the aux loss a unit gradient scaled by
    `coeff`, so stages before the pipeline's loss stage still train their
    routers under 1F1B."""

    @staticmethod
    def forward(ctx, x, aux, coeff):
        ctx.coeff = coeff
        return x

    @staticmethod
    def backward(ctx, dy):
        return dy, dy.new_tensor(ctx.coeff * _AUX_LOSS_SCALE), None


def attach_aux_loss(x: torch.Tensor, aux: torch.Tensor, coeff: float):
    return _AttachAuxLoss.apply(x, aux, coeff)


def load_balancing_loss_func(router_logits: torch.Tensor, num_experts: int,
                             top_k: int) -> torch.Tensor:
    """Switch-style aux loss: num_experts * sum_e f_e * P_e
    (reference modeling_mixtral.py:872-888 contract)."""
    probs = torch.softmax(router_logits.float(), dim=-1)  # [T, E]
    _, sel = probs.topk(top_k, dim=-1)
    onehot = torch.zeros_like(probs).scatter_(1, sel, 1.0)
    tokens_per_expert = onehot.mean(0)  # f_e * top_k
    prob_per_expert = probs.mean(0)     # P_e
    return num_experts * (tokens_per_expert * prob_per_expert).sum() / top_k


class RouterTopK(nn.Module):
    """Top-k router (reference RouterTopK contract incl. the
    ``act_fn`` softmax/sigmoid and ``normalize_top_k_affinities`` knobs,
    transformer.py:402-431)."""

    def __init__(self, hidden_size: int, num_experts: int, top_k: int,
                 dtype: torch.dtype = torch.float32, init_seed: Optional[int] = None,
                 act_fn: str = "softmax", normalize_top_k_affinities: bool = True):
        super().__init__()
        self.num_experts = num_experts
        self.top_k = top_k
        assert act_fn in ("softmax", "sigmoid"), act_fn
        self.act_fn = act_fn
        self.normalize_top_k_affinities = normalize_top_k_affinities
        if init_seed is not None:
            st = torch.random.get_rng_state()
            torch.manual_seed(init_seed)
        w = torch.empty(num_experts, hidden_size, dtype=torch.float32)
        nn.init.normal_(w, std=0.02)
        if init_seed is not None:
            torch.random.set_rng_state(st)
        self.weight = nn.Parameter(w.to(dtype))

    def forward(self, x: torch.Tensor):
        """x: [T, H] → (weights [T, k], indices [T, k], logits [T, E])."""
        logits = F.linear(x, self.weight).float()
        if self.act_fn == "sigmoid":
            probs = torch.sigmoid(logits)
        else:
            probs = torch.softmax(logits, dim=-1)
        topw, topi = probs.topk(self.top_k, dim=-1)
        if self.normalize_top_k_affinities:
            topw = topw / topw.sum(dim=-1, keepdim=True)
        return topw.to(x.dtype), topi, logits


class RouterSinkhorn(RouterTopK):
    """Sinkhorn-balanced routing (reference RouterSinkhorn contract)."""

    def __init__(self, *args, n_iter: int = 3, tol: Optional[float] = None, **kw):
        super().__init__(*args, **kw)
        self.n_iter = n_iter
        self.tol = tol  # early-exit threshold (reference moe_sinkhorn_tol)

    def forward(self, x: torch.Tensor):
        logits = F.linear(x, self.weight).float()
        with torch.no_grad():
            cost = torch.exp(logits)
            d0 = torch.ones(cost.size(0), device=cost.device)
            d1 = torch.ones(cost.size(1), device=cost.device)
            eps = 1e-8
            for _ in range(self.n_iter):
                d1_old = d1
                d0 = 1.0 / (cost @ d1 + eps)
                d1 = cost.size(0) / cost.size(1) / (cost.t() @ d0 + eps)
                if self.tol is not None and float(
                    (d1 - d1_old).abs().max()
                ) < self.tol:
                    break
            balanced = cost * d0.unsqueeze(1) * d1.unsqueeze(0)
            _, topi = balanced.topk(self.top_k, dim=-1)
        # gradients flow through softmax of raw logits at chosen experts
        probs = torch.softmax(logits, dim=-1)
        topw = probs.gather(-1, topi)
        topw = topw / topw.sum(dim=-1, keepdim=True)
        return topw.to(x.dtype), topi, logits


class ExpertMLPs(nn.Module):
    """Local shard of the expert set: num_experts/ep SwiGLU MLPs.

    Weights are stacked [E_local, ...] so the dropless path runs one
    GEMM per local expert over its sorted token slab.
    """

    def __init__(self, num_experts: int, hidden_size: int,
                 intermediate_size: int, dtype: torch.dtype = torch.float32,
                 init_seed: Optional[int] = None):
        super().__init__()
        ep = ps.get_expert_model_parallel_world_size()
        ep_rank = ps.get_expert_model_parallel_rank()
        assert num_experts % ep == 0
        self.num_experts = num_experts
        self.num_local = num_experts // ep
        self.local_offset = ep_rank * self.num_local
        self.hidden_size = hidden_size
        self.intermediate_size = intermediate_size

        if init_seed is not None:
            st = torch.random.get_rng_state()
            torch.manual_seed(init_seed)
        gu = torch.empty(num_experts, 2 * intermediate_size, hidden_size)
        dn = torch.empty(num_experts, hidden_size, intermediate_size)
        nn.init.normal_(gu, std=0.02)
        nn.init.normal_(dn, std=0.02)
        if init_seed is not None:
            torch.random.set_rng_state(st)
        sl = slice(self.local_offset, self.local_offset + self.num_local)
        self.gate_up = nn.Parameter(gu[sl].to(dtype))
        self.down = nn.Parameter(dn[sl].to(dtype))
        self.gate_up.expert_model_parallel = True
        self.down.expert_model_parallel = True

    def grouped_chosen(self, x: torch.Tensor, rows: int):
        """Whether `rows` expert-sorted rows with x's dtype, device and width
        go to the grouped HIP kernel (truthy) or to the library path: the
        kernel must take the operands, and NXDT_MOE_GROUPED=1/0 forces;
        unforced, grouped runs up to 1024 rows per local expert."""
        from ..ops.moe_gemm import grouped_path_supported

        force = os.environ.get("NXDT_MOE_GROUPED", "")
        return (
            rows * x.size(-1)
            and grouped_path_supported(x, self.gate_up, self.down)
            and (
                force == "1"
                or (force != "0"
                    and rows <= 1024 * self.num_local)
            )
        )

    def forward(self, x: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
        """x: [T, H] tokens sorted by local expert; counts: [E_local] token
        counts per local expert. Returns same-order outputs.

        On GPU the grouped-GEMM HIP kernel runs all experts in one launch
        per projection with DEVICE-side layout math — no per-expert loop,
        no .tolist() host sync. Measured on MI355X
        (Mixtral 8x7B shape, fwd+bwd, tools/bench_moe_layer.py): grouped
        is 2.3x at ~128 tokens/expert, 1.4x at ~512, and 0.87x at ~2k,
        where hipBLASLt's per-GEMM throughput wins — so the grouped path
        runs below GROUPED_MAX_TOKENS_PER_EXPERT and the library path
        (bmm / per-expert loop) above. NXDT_MOE_GROUPED=1/0 forces."""
        from ..ops.moe_gemm import grouped_expert_mlp

        if self.grouped_chosen(x, x.size(0)):
            return grouped_expert_mlp(x, counts, self.gate_up, self.down)
        cl = counts.tolist()
        total = int(sum(cl))
        if total == 0:
            return x.new_zeros(0, self.hidden_size)
        cap = max(cl)
        if self.num_local > 1 and cap * self.num_local <= max(
            int(1.25 * total), total + self.num_local
        ):
            return self._forward_bmm(x, cl, cap)
        outs = []
        start = 0
        for e in range(self.num_local):
            n = cl[e]
            if n == 0:
                continue
            xe = x[start : start + n]
            h = F.linear(xe, self.gate_up[e])
            h = swiglu(h)
            outs.append(F.linear(h, self.down[e]))
            start += n
        return torch.cat(outs, dim=0)

    def _forward_bmm(self, x, cl, cap):
        # scatter the sorted slab into a padded [E, cap, H] cube, run two
        # bmms, gather the real rows back in order
        E = self.num_local
        idx = torch.cat([
            torch.arange(e * cap, e * cap + n, device=x.device)
            for e, n in enumerate(cl)
        ])
        cube = x.new_zeros(E * cap, x.size(-1))
        cube[idx] = x
        h = torch.bmm(cube.view(E, cap, -1), self.gate_up.transpose(1, 2))
        h = swiglu(h)
        out = torch.bmm(h, self.down.transpose(1, 2))
        return out.reshape(E * cap, self.hidden_size)[idx]


class MoE(nn.Module):
    """Router + (optional EP all-to-all) + expert MLPs + combine.

    Dropless by default; with ``capacity_factor`` set, tokens beyond
    capacity per expert are dropped (their MoE output is 0 — residual
    carries them, matching capacity-factor semantics).

    NXDT_MOE_FUSED=1 (read per call, default 0; any other value raises a
    ValueError) replaces the chain of torch index ops between the router and
    the output with the HIP token path of ops.moe_dispatch (plan, permute,
    grouped expert MLP in the padded layout, fp32 combine), in dropless and
    capacity mode alike. It applies with EP = 1, at most 64 experts and
    top-8, where ExpertMLPs would choose the grouped kernel for the T * k
    rows (in capacity mode the eager path asks that of the kept rows, this
    one of all T * k: the kept count lives on the device); everywhere else,
    CPU included, the layer runs the eager code unchanged. The same pairs are
    kept and the same experts applied; the combine and its backward round
    once in fp32 where eager rounds per pair in bf16.
    """

    def __init__(self, router: RouterTopK, experts: ExpertMLPs,
                 capacity_factor: Optional[float] = None,
                 token_shuffle_group_size: int = 1,
                 moe_dropout: float = 0.0):
        super().__init__()
        self.router = router
        self.experts = experts
        self.capacity_factor = capacity_factor
        self.token_shuffle_group_size = token_shuffle_group_size
        self.dropout = nn.Dropout(moe_dropout) if moe_dropout else None
        self.ep = ps.get_expert_model_parallel_world_size()

    def _fused_path(self, x: torch.Tensor, k: int, E: int) -> bool:
        from ..ops import moe_fused
        from ..ops.moe_dispatch import MAX_EXPERTS, MAX_TOP_K

        return bool(
            moe_fused()   # raises on an invalid NXDT_MOE_FUSED, taken or not
            and self.ep == 1
            and E <= MAX_EXPERTS and k <= MAX_TOP_K
            and self.experts.grouped_chosen(x, x.size(0) * k)
        )

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x: [T, H] (caller flattens [s,b,h]). Returns (y [T, H],
        router_logits [T, E] — computed on the shuffled token order when
        token_shuffle_group_size > 1; the aux loss is order-invariant)."""
        shuf_ctx = None
        if self.token_shuffle_group_size > 1:
            x, shuf_ctx = token_shuffle(x, self.token_shuffle_group_size)
        T, H = x.shape
        k = self.router.top_k
        E = self.router.num_experts
        topw, topi, logits = self.router(x)

        if self._fused_path(x, k, E):
            from ..ops.moe_dispatch import fused_moe_experts

            cap = (int(math.ceil(self.capacity_factor * T * k / E))
                   if self.capacity_factor else 0)
            y = fused_moe_experts(x, topw, topi, self.experts.gate_up,
                                  self.experts.down, cap)
            if self.dropout is not None:
                y = self.dropout(y)
            if shuf_ctx is not None:
                y = token_unshuffle(y, shuf_ctx)
            return y, logits

        # flatten (token, choice) pairs
        flat_exp = topi.reshape(-1)                   # [T*k]
        flat_tok = (
            torch.arange(T, device=x.device).repeat_interleave(k)
        )
        flat_w = topw.reshape(-1)

        if self.capacity_factor:
            cap = int(math.ceil(self.capacity_factor * T * k / E))
            # rank within each expert queue; drop beyond capacity
            sort_by_e = torch.argsort(flat_exp, stable=True)
            sorted_e = flat_exp[sort_by_e]
            ones = torch.ones_like(sorted_e)
            pos_in_e = torch.cumsum(ones, 0) - 1
            seg_start = torch.searchsorted(sorted_e, torch.arange(E, device=x.device))
            pos_in_e = pos_in_e - seg_start[sorted_e]
            keep_sorted = pos_in_e < cap
            keep = torch.zeros_like(keep_sorted)
            keep[sort_by_e] = keep_sorted
            flat_exp = flat_exp[keep]
            flat_tok = flat_tok[keep]
            flat_w = flat_w[keep]

        order = torch.argsort(flat_exp, stable=True)
        sorted_exp = flat_exp[order]
        sorted_tok = flat_tok[order]
        sorted_w = flat_w[order]
        counts = torch.bincount(sorted_exp, minlength=E)  # [E]

        xin = x[sorted_tok]  # gathered inputs, expert-sorted

        if self.ep > 1:
            group = ps.get_expert_model_parallel_group()
            nl = self.experts.num_local
            # tokens destined for rank r = those routed to experts [r*nl,(r+1)*nl)
            send_counts = counts.view(self.ep, nl).sum(-1)
            recv_counts = torch.empty_like(send_counts)
            dist.all_to_all_single(recv_counts, send_counts, group=group)
            in_splits = send_counts.tolist()
            out_splits = recv_counts.tolist()
            # per-(src, local_expert) counts
            counts_mat = torch.empty(self.ep * nl, dtype=counts.dtype,
                                     device=counts.device)
            dist.all_to_all_single(counts_mat, counts.contiguous(), group=group)
            counts_mat = counts_mat.view(self.ep, nl)

            xrecv = _AllToAll.apply(xin.contiguous(), out_splits, in_splits, group)
            # received rows arrive [src][expert]-ordered; resort expert-major
            eids = torch.cat(
                [
                    torch.repeat_interleave(
                        torch.arange(nl, device=x.device), counts_mat[r]
                    )
                    for r in range(self.ep)
                ]
            ) if xrecv.size(0) else torch.zeros(0, dtype=torch.long, device=x.device)
            order2 = torch.argsort(eids, stable=True)
            local_counts = counts_mat.sum(0)
            yloc = self.experts(xrecv[order2], local_counts)
            inv = torch.empty_like(order2)
            inv[order2] = torch.arange(order2.numel(), device=x.device)
            back = yloc[inv]
            yexp = _AllToAll.apply(back.contiguous(), in_splits, out_splits, group)
        else:
            yexp = self.experts(xin, counts)

        # combine: scatter-add weighted expert outputs back to tokens
        y = torch.zeros_like(x)
        y.index_add_(0, sorted_tok, yexp * sorted_w.unsqueeze(-1))
        if self.dropout is not None:
            y = self.dropout(y)
        if shuf_ctx is not None:
            y = token_unshuffle(y, shuf_ctx)
        return y, logits
